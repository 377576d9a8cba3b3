"""Exact tests of the split-operand GEMMs (csrc/gemm_split.hip) on every kernel instantiation and edge; run with -m gpu.

Operands, reference and the argument for exactness: tests/gemm_exact_ref.py.  Every case must return the reference BIT
FOR BIT (torch.equal): there is no tolerance.  Operands are views inside NaN-filled buffers (NaN rows before and after,
NaN in the columns K..ld of every row), outputs sit in NaN guard bands and the scratch is prefilled with NaN, so a read
outside an operand that is multiplied by zero instead of being selected away, or a store outside C, shows too.

CASES is built by design, not by accident: for each of the 24 instantiations (form x pieces x tile width, + the
residual variant of the two-piece nt / nn) one case per regime the form admits.  tests/test_gemm_exact_cpu.py plans the
list with sigma_gemm_plan (no GPU) and fails when an instantiation, a regime or an epilogue x store combination is not
reached, or when a case does not plan to the variant it names.
"""
import itertools

import pytest
import torch

from tests.gemm_exact_ref import Case, exact_operand, exact_product, run_case, describe_mismatch, unit_multiples, pieces_of, unit_of

DEV = "cuda"

FORMS = ("nt", "nn", "tn")
WIDTHS = (128, 96, 64)
# every kernel the launch code instantiates: (form, pieces, tile width, residual variant)
INSTANTIATIONS = [(f, P, bn, False) for f in FORMS for P in (2, 3) for bn in WIDTHS] + [(f, 2, bn, True) for f in ("nt", "nn") for bn in WIDTHS]

# kernel columns that pick_bn maps to each width: one full tile, a ragged multiple of 4, and (nt only) N % 4 != 0
COLS_FULL = {128: 128, 96: 96, 64: 64}
COLS_RAGGED = {128: 200, 96: 76, 64: 36}
COLS_ODD = {128: 198, 96: 70, 64: 30}


def _density(P, kr, kind=None, outputs=0):
    """share of nonzero elements per operand such that a reduction of kr stays in the 2^24 window with margin (the
    builder asserts the window; this only has to be safe): three pieces hold ~15 full products, 'wide' ~1800, 'unit' ~16000"""
    if P == 3 and kr <= 12:
        return (1.0, 1.0)
    cap = (3.0 if outputs < 1e5 else 1.5) if P == 3 else (1300.0 if kind != "unit" else 14000.0)
    d = min(1.0, (cap / kr) ** 0.5)
    return (d, d)


def _api(form, mr, nc, kr):
    """kernel view (rows, columns, reduction) -> M, N, K of sigma_gemm_params"""
    return (kr, mr, nc) if form == "tn" else (mr, nc, kr)


def _case(tag, inst, mr, nc, kr, **kw):
    form, P, bn, res = inst
    M, N, K = _api(form, mr, nc, kr)
    kw.setdefault("res", 1 if res else 0)
    batch, c_mod = kw.get("batch", 1), kw.get("c_mod", 0)
    groups = -(-batch // c_mod) if 0 < c_mod < batch else 1           # problems summed into one output
    kw.setdefault("density", _density(P, kr * groups, kw.get("kind"), batch * mr * nc))
    name = f"{form}{P}-{bn}{'r' if res else ''}-{tag}"
    return Case(name=name, form=form, M=M, N=N, K=K, pieces=P, variant=(bn, res), seed=len(name) + sum(map(ord, name)), **kw)


def _cases_of(inst):
    form, P, bn, res = inst
    full, rag, odd = COLS_FULL[bn], COLS_RAGGED[bn], COLS_ODD[bn]
    lin = form != "tn"                        # nt / nn: bias, a_mod, c_mod, residuals
    r2 = 130 if lin else 132                  # two row tiles, the second ragged (tn: rows of C % 4 == 0)
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))
    # (a) one full tile, whole k-steps
    add("a-full", inst, 128, full, 64)
    # (b) ragged rows and columns, partial k-steps
    add("b-ragged-k68", inst, r2, rag, 68, bias=lin)
    add("b-ragged-k60-acc", inst, 40, rag, 60, accumulate=True)
    add("b-k12", inst, 20, full, 12)
    if form == "nt":
        add("b-m1", inst, 1, odd, 8)
        add("b-m17-odd", inst, 17, odd, 100, bias=True)
    # (c) more items than the persistent grid holds (2080, the grid is at most 1024): five row tiles per problem, the last one ragged; a
    # workgroup steps through the item ids by a multiple of 8 that 5 does not divide, so full and ragged tiles alternate
    # along its stream and the operand ring crosses both kinds of boundary
    add("c-persistent", inst, 520, full, 36, batch=416, kind="unit" if P == 2 else None)
    # (d) sliced reductions with a ragged last slice
    if form != "nt" and not res:
        ks = dict(k_slices=1) if form == "nn" else {}
        add("d-two-stage", inst, 40, rag, 516, **ks)
        add("d-atomic-zero", inst, 40, rag, 516, ws="none", **ks)
        add("d-atomic-acc", inst, 40, rag, 516, ws="none", accumulate=True, **ks)
        add("d-short-scratch", inst, 40, rag, 516, ws="short", **ks)
        add("d-two-stage-acc", inst, 132, full, 516, accumulate=True, **ks)
    # (e) stacked problems
    if lin:
        add("e-a_mod", inst, 40, rag, 36, batch=4, a_mod=2, bias=True)
        add("e-a_mod-rows2", inst, r2, rag, 36, batch=4, a_mod=2, res=2 if res else 0)      # the stacked projections of the scan core
        if not res:
            add("e-c_mod-exact", inst, 40, rag, 36, batch=4, c_mod=2)
            add("e-c_mod-exact-acc", inst, 40, rag, 36, batch=6, c_mod=3, accumulate=True)
            add("e-c_mod-ragged", inst, 40, rag, 36, batch=5, c_mod=2)
            add("e-c_mod-ragged-atomic", inst, 40, rag, 36, batch=5, c_mod=2, ws="none")
        add("e-c_mod-ge-batch", inst, 40, rag, 36, batch=2, c_mod=4)
    else:
        add("e-batch", inst, 40, rag, 36, batch=3)
    # (f) epilogues: the direct one by each of its causes, both store modes
    add("f-direct-ldc", inst, r2, rag, 36, pad=(4, 8, 5, 4), bias=lin)
    add("f-direct-misaligned-acc", inst, 40, rag, 36, c_off=1, accumulate=True)
    add("f-direct-strideC", inst, 40, rag, 36, batch=2, sC_pad=2)
    if form == "nt":
        add("f-direct-n4-acc", inst, r2, odd, 36, accumulate=True, bias=True)
    if res:
        add("f-res2-vector", inst, r2, rag, 36, res=2, bias=True)
        add("f-res1-scalar-ldr", inst, r2, rag, 36, res=1, pad=(4, 8, 4, 5))
        add("f-res2-scalar-misaligned", inst, 40, rag, 36, res=2, r_off=1, accumulate=True)
        add("f-res2-batch", inst, 40, rag, 36, res=2, batch=3, a_mod=0)
        add("f-res1-scalar-strideR", inst, 40, rag, 36, res=1, batch=2, sR_pad=2)
        if form == "nt":
            add("f-res1-scalar-n4", inst, r2, odd, 36, res=1)
    if form == "nt" and not res:
        add("f-t_cols-eq", inst, 40, full, 36, t_cols=full, bias=True)
        add("f-t_cols-straddle", inst, 132, full, 36, t_cols=32)
        if bn != 64:
            add("f-t_cols-tile", inst, 40, 2 * full, 36, t_cols=full)
    return out


def _epilogue_product():
    """(f) every combination of epilogue kind x store mode x bias x residuals the plan functions admit, once, on the
    narrow two-piece kernels of nt and nn (one ragged tile each)"""
    out = []
    for form in ("nt", "nn"):
        for direct, acc, bias, (nres, scalar) in itertools.product((False, True), (False, True), (False, True),
                                                                  ((0, False), (1, False), (2, False), (1, True), (2, True))):
            inst = (form, 2, 64, nres > 0)
            tag = f"fx-{'direct' if direct else 'rows'}-{'acc' if acc else 'store'}-{'bias' if bias else 'nobias'}-res{nres}{'s' if scalar else 'v' if nres else ''}"
            out.append(_case(tag, inst, 40, 36, 36, accumulate=acc, bias=bias, res=nres, pad=(4, 8, 5 if direct else 4, 5 if scalar else 4)))
    for bias in (False, True):
        out.append(_case(f"fx-t_cols-{'bias' if bias else 'nobias'}", ("nt", 2, 64, False), 40, 64, 36, t_cols=32, bias=bias))
    return out


def _real_shapes():
    """(g) the shapes of the training step (sigma_small, 480 x 640), once each"""
    u = dict(kind="unit")
    c = lambda tag, form, bn, M, N, K, has_res=False, **kw: Case(name=f"{form}2-{bn}{'r' if has_res else ''}-g-{tag}", form=form, M=M, N=N, K=K,
                                                                 variant=(bn, has_res), seed=len(tag), **kw)
    return [
        c("in_proj", "nt", 128, 19200, 1536, 384, **u),
        c("in_proj-bias", "nt", 128, 19200, 1536, 384, bias=True, **u),
        c("in_proj-t_cols", "nt", 128, 19200, 1536, 384, bias=True, t_cols=768, **u),
        c("dgrad", "nn", 128, 19200, 384, 1536, **u),
        c("wgrad-s2", "tn", 128, 19200, 1536, 384, density=(0.9, 0.9), **u),
        c("wgrad-decoder", "tn", 96, 76800, 384, 96, density=(0.5, 0.4), **u),
        # CORE_SHAPES[0] of tests/test_gemm_gpu.py, (B, d, c, R, L) = (2, 768, 56, 24, 1200): x_proj, dt_proj, the x_proj input
        # gradient with the scan's two du, the x_proj weight gradient summed over the batch
        c("x_proj", "nn", 96, 112, 1200, 768, batch=4, a_mod=2),
        c("dt_proj", "nn", 96, 768, 1200, 24, batch=8, a_mod=4),
        c("x_proj-dgrad", "nn", 96, 768, 1200, 112, has_res=True, batch=4, a_mod=2, res=2),
        c("x_proj-wgrad", "nt", 128, 112, 768, 1200, batch=4, c_mod=2, accumulate=True, density=(0.7, 0.7)),
    ]


CASES = [c for inst in INSTANTIATIONS for c in _cases_of(inst)] + _epilogue_product() + _real_shapes()
assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_exact_case(case):
    """the launch returns the int / fp64 reference bit for bit, free of NaN, and writes nothing outside its outputs"""
    got, want, rep = run_case(case, DEV)
    print(f"{case.name}: {rep['plan']} unit {rep['unit']} window fill {rep['fill']:.3f}")
    assert not bool(torch.isnan(got).any()) and torch.equal(got.double(), want), f"{case.name}: " + describe_mismatch(got, want, rep["unit"])


# ---------------------------------------------------------------------------------------------------------------------
# the same arithmetic through the Python wrappers (strides and _params plumbing), exact too

def _ops(form, M, N, K, P=2, batch=1, za=None, seed=0, kind=None, density=(1.0, 1.0)):
    c = Case(name="w", form=form, M=M, N=N, K=K, pieces=P, batch=batch, a_mod=za or 0, seed=seed, kind=kind, density=density)
    o = c.operands()
    return o["A"].to(DEV), o["B"].to(DEV), o["unit"]


def _exact(got, want, what):
    assert not bool(torch.isnan(got).any()) and torch.equal(got.double(), want), f"{what}: {int((got.double() != want).sum())} of {got.numel()} differ"


@pytest.mark.gpu
def test_wrappers_nt_exact():
    from sigma_amd import gemm
    for M, N, K in ((130, 200, 68), (257, 70, 100)):
        A, B, unit = _ops("nt", M, N, K, seed=M)
        bias = unit_multiples((N,), unit, 5).to(DEV)
        r = unit_multiples((1, M, N), unit, 6).to(DEV)
        want, _, _ = exact_product("nt", A, B, 2, bias=bias)
        _exact(gemm.gemm_nt(A[0], B[0], bias), want[0], f"gemm_nt {M}x{N}x{K}")
        want, _, _ = exact_product("nt", A, B, 2, residuals=(r,))
        _exact(gemm.gemm_nt(A[0], B[0], residual=r[0]), want[0], f"gemm_nt residual N={N}")          # N = 70: scalar residual loads
        wide = torch.full((M, N + 10), float("nan"), device=DEV)
        view = wide[:, 3:3 + N]                                                                       # misaligned, ldc % 4 != 0
        old = unit_multiples((1, M, N), unit, 7).to(DEV)
        view.copy_(old[0])
        want, _, _ = exact_product("nt", A, B, 2, old=old)
        gemm.gemm_nt(A[0], B[0], out=view, accumulate=True)
        _exact(view, want[0], f"gemm_nt out=view accumulate N={N}")                                  # direct epilogue with accumulate
        assert bool(torch.isnan(wide[:, :3]).all()) and bool(torch.isnan(wide[:, 3 + N:]).all())
    A, B, unit = _ops("nt", 40, 76, 12, P=3, seed=3)
    _exact(gemm.gemm_nt(A[0], B[0], pieces=3), exact_product("nt", A, B, 3)[0][0], "gemm_nt three pieces")


@pytest.mark.gpu
def test_wrappers_nn_tn_exact():
    from sigma_amd import gemm
    A, B, unit = _ops("nn", 130, 76, 68, seed=1)
    _exact(gemm.gemm_nn(A[0], B[0]), exact_product("nn", A, B, 2)[0][0], "gemm_nn")
    A, B, unit = _ops("nn", 40, 36, 1028, seed=2)
    want = exact_product("nn", A, B, 2)[0][0]
    _exact(gemm.gemm_nn(A[0], B[0], k_slices=True), want, "gemm_nn k_slices")
    old = unit_multiples((1, 40, 36), unit, 9).to(DEV)
    got = gemm.gemm_nn(A[0], B[0], out=old[0].clone(), accumulate=True, k_slices=True)
    _exact(got, exact_product("nn", A, B, 2, old=old)[0][0], "gemm_nn k_slices accumulate")
    A, B, unit = _ops("tn", 1028, 40, 36, seed=3)
    want = exact_product("tn", A, B, 2)[0][0]
    big = torch.full((80, 36), float("nan"), device=DEV)
    gemm.gemm_tn(A[0], B[0], out=big[40:])
    _exact(big[40:], want, "gemm_tn into a view")
    assert bool(torch.isnan(big[:40]).all())
    old = unit_multiples((1, 40, 36), unit, 10).to(DEV)
    _exact(gemm.gemm_tn(A[0], B[0], out=old[0].clone(), accumulate=True), exact_product("tn", A, B, 2, old=old)[0][0], "gemm_tn accumulate")


@pytest.mark.gpu
def test_wrappers_stacked_exact():
    from sigma_amd import gemm
    Z, Za, M, K, N = 4, 2, 40, 36, 76
    A, B, unit = _ops("nn", M, N, K, batch=Z, za=Za, seed=4)
    r1, r2 = (unit_multiples((Z, M, N), unit, s).to(DEV) for s in (11, 12))
    out = torch.full((Z, M + 4, N), float("nan"), device=DEV)[:, :M]                                   # row-slice views
    gemm.bgemm_nn(A, B, out)
    _exact(out, exact_product("nn", A, B, 2, a_mod=Za)[0], "bgemm_nn")
    gemm.bgemm_nn(A, B, out, residual=r1, residual2=r2)
    _exact(out, exact_product("nn", A, B, 2, a_mod=Za, residuals=(r1, r2))[0], "bgemm_nn residuals")
    A, B, unit = _ops("nt", M, N, K, batch=Z, seed=5)
    old = unit_multiples((2, M, N), unit, 13).to(DEV)
    got = gemm.bgemm_nt_sum(A, B, old.clone())
    _exact(got, exact_product("nt", A, B, 2, c_mod=2, old=old)[0], "bgemm_nt_sum accumulate")
    got = gemm.bgemm_nt_sum(A, B, torch.full((2, M, N), float("nan"), device=DEV), accumulate=False)
    _exact(got, exact_product("nt", A, B, 2, c_mod=2)[0], "bgemm_nt_sum overwrite")


@pytest.mark.gpu
def test_wrappers_linear_forward_and_backward_exact():
    """gemm.linear and gemm.linear_xz: y, dx, dW (and db, a plain sum of integers) are exact on exact operands"""
    from sigma_amd import gemm
    M, K, N = 136, 68, 128
    x = exact_operand((1, M, K), 2, 21).to(DEV)
    w = exact_operand((1, N, K), 2, 22).to(DEV)
    dy = exact_operand((1, M, N), 2, 23).to(DEV)
    unit = unit_of(pieces_of(x, 2), pieces_of(w, 2))
    b = unit_multiples((N,), unit, 24).to(DEV)
    r = unit_multiples((1, M, N), unit, 25).to(DEV)
    xa, wa, ba, ra = (t.clone().requires_grad_() for t in (x, w[0], b, r))
    y = gemm.linear(xa, wa, ba, residual=ra)
    _exact(y.detach(), exact_product("nt", x, w, 2, bias=b, residuals=(r,))[0], "linear forward")
    y.backward(dy)
    _exact(xa.grad, exact_product("nn", dy, w, 2)[0], "linear dx")
    _exact(wa.grad, exact_product("tn", dy, x, 2)[0][0], "linear dW")
    _exact(ba.grad, dy[0].double().sum(0), "linear db")
    assert torch.equal(ra.grad, dy)
    # in_proj with the channel-major x half: (B, H, W, C) = (1, 4, 10, 68), d = 64
    Bn, H, W, C, d = 1, 4, 10, 68, 64
    x = exact_operand((1, Bn * H * W, C), 2, 31).to(DEV)
    w = exact_operand((1, 2 * d, C), 2, 32).to(DEV)
    unit = unit_of(pieces_of(x, 2), pieces_of(w, 2))
    b = unit_multiples((2 * d,), unit, 33).to(DEV)
    xa, wa, ba = x.view(Bn, H, W, C).clone().requires_grad_(), w[0].clone().requires_grad_(), b.clone().requires_grad_()
    assert gemm.xz_ok(xa.reshape(-1, C), wa)
    xi, z = gemm.linear_xz(xa, wa, ba)
    want = exact_product("nt", x, w, 2, bias=b)[0][0]
    _exact(xi.detach().permute(0, 2, 3, 1).reshape(-1, d), want[:, :d], "linear_xz x half")
    _exact(z.detach().reshape(-1, d), want[:, d:], "linear_xz z half")
    g = exact_operand((1, Bn * H * W, 2 * d), 2, 34).to(DEV)
    gx = g[0, :, :d].reshape(Bn, H, W, d).permute(0, 3, 1, 2)
    gz = g[0, :, d:].reshape(Bn, H, W, d)
    torch.autograd.backward((xi, z), (gx, gz))
    # dx = dz W_z + dxT^T W_x: two launches, the second accumulating -- the sum of two exact products inside one window
    dxz = exact_product("nn", g[:, :, d:].contiguous(), w[:, d:].contiguous(), 2)[0]
    dx = exact_product("nn", g[:, :, :d].contiguous(), w[:, :d].contiguous(), 2, old=dxz[0].float().unsqueeze(0))[0]
    _exact(xa.grad.reshape(-1, C), dx[0], "linear_xz dx")
    _exact(wa.grad, exact_product("tn", g, x, 2)[0][0], "linear_xz dW")
    _exact(ba.grad, g[0].double().sum(0), "linear_xz db")
