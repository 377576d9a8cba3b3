"""GPU parity tests of the split-operand bf16 MFMA GEMMs (csrc/gemm_split.hip, include/sigma_gemm.h; run with -m gpu).

Checker: the same product in fp64 (torch on the GPU).  A product of fp32 operands split into (hi, lo) bf16 pairs with the
lo*lo term dropped has a relative error of ~2^-16 per product term at worst and ~4e-6 rms on sums; the bound used here is
3e-5 * sum_k |a||b| per output element (the fp32 library GEMM sits at ~1e-6 of the same scale).  The model-level
tolerance (1e-3 on logits, the reference's gradient tolerances) is checked in tests/test_model_gpu.py with these kernels on.

The last section plants NaN, +-inf, magnitudes at the bf16 overflow edge and very small magnitudes in operand elements
and pins which elements of C they may touch.  Those tests only detect: non-finite VALUES are data, not addresses, and no
test makes a kernel read or write outside memory the test owns.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(DEV)


def _bound(a64, b64):
    """sum_k |a||b| per output element for C = a @ b (both given in product orientation (M, K) x (K, N))"""
    return a64.abs() @ b64.abs()


def _assert_close(got, want64, bound, what):
    err = (got.double() - want64).abs()
    worst = float((err / (bound + 1e-30)).max())
    assert worst < 3e-5, f"{what}: max error / sum|a||b| = {worst:.3e}"
    rms = float(err.pow(2).mean().sqrt() / want64.pow(2).mean().sqrt())
    assert rms < 2e-5, f"{what}: relative rms error {rms:.3e}"


NT_SHAPES = [
    # (M, K, N): in_proj / out_proj / PatchMerging / decoder shapes of sigma_small at 480x640 plus ragged ones
    (19200, 384, 1536), (19200, 768, 384), (4800, 192, 768), (1200, 1536, 768), (2400, 96, 384), (3000, 192, 96),
    (300, 768, 1536), (257, 100, 70), (128, 32, 128), (5, 4, 3), (1, 8, 1), (130, 36, 200),
]


@pytest.mark.parametrize("shape", NT_SHAPES, ids=["x".join(map(str, s)) for s in NT_SHAPES])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_gemm_nt_against_fp64(shape, with_bias):
    from sigma_amd import gemm
    M, K, N = shape
    a, w = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=0.05)
    bias = _rand(N, seed=3) if with_bias else None
    got = gemm.gemm_nt(a, w, bias)
    want = a.double() @ w.double().t() + (bias.double() if with_bias else 0.0)
    _assert_close(got, want, _bound(a.double(), w.double().t()), "nt")


@pytest.mark.parametrize("shape", [(19200, 384, 1536), (300, 768, 1536), (18, 768, 1536), (18, 1536, 768), (6, 768, 1536), (792, 96, 384),
                                   (257, 100, 70), (5, 4, 3)], ids=lambda s: "x".join(map(str, s)))
def test_three_piece_gemms_reach_fp32_accuracy(shape):
    """pieces = 3 (hi, mid, lo: six MFMAs per block): error against fp64 at the level of an fp32 GEMM (~1e-6 of
    sum |a||b|), for the forward (nt), the input gradient (nn) and the weight gradient (tn)."""
    from sigma_amd import gemm
    M, K, N = shape
    a, w = _rand(M, K, seed=21), _rand(N, K, seed=22, scale=0.05)
    bias = _rand(N, seed=23)
    def check(got, want, bound, what):
        worst = float(((got.double() - want).abs() / (bound + 1e-30)).max())
        assert worst < 2e-6, f"{what}: max error / sum|a||b| = {worst:.3e}"
    check(gemm.gemm_nt(a, w, bias, pieces=3), a.double() @ w.double().t() + bias.double(), _bound(a.double(), w.double().t()), "nt p3")
    if N % 4 == 0 and K % 4 == 0:
        dy = _rand(M, N, seed=24)
        check(gemm.gemm_nn(dy, w, pieces=3), dy.double() @ w.double(), _bound(dy.double(), w.double()), "nn p3")
        check(gemm.gemm_tn(dy, a, pieces=3), dy.double().t() @ a.double(), _bound(dy.double().t(), a.double()), "tn p3")


def test_gemm_nt_is_not_transposed_identity_check():
    """A = I with an ASYMMETRIC B: catches a row/column swap in the accumulator write (a symmetric B would not)."""
    from sigma_amd import gemm
    n = 160
    a = torch.eye(n, device=DEV)
    w = (torch.arange(n * n, device=DEV, dtype=torch.float32).view(n, n) % 251) / 16.0      # exactly representable in bf16 x 2
    got = gemm.gemm_nt(a, w)                                      # C = I @ w^T
    assert torch.equal(got, w.t().contiguous())


def test_gemm_nt_strided_operands_accumulate_and_out():
    """A as the x half of an in_proj output (row stride 2K), out as a column slice of a wider buffer, accumulate."""
    from sigma_amd import gemm
    M, K, N = 1000, 192, 96
    xz = _rand(M, 2 * K, seed=4)
    a = xz[:, :K]
    w = _rand(N, K, seed=5, scale=0.1)
    wide = torch.zeros(M, 2 * N, device=DEV)
    out = wide[:, N:]
    gemm.gemm_nt(a, w, out=out)
    want = a.double() @ w.double().t()
    _assert_close(out, want, _bound(a.double(), w.double().t()), "nt strided")
    assert float(wide[:, :N].abs().max()) == 0.0
    gemm.gemm_nt(a, w, out=out, accumulate=True)
    _assert_close(out, 2 * want, 2 * _bound(a.double(), w.double().t()), "nt accumulate")


@pytest.mark.parametrize("shape", [(19200, 1536, 384), (19200, 384, 768), (4800, 96, 192), (300, 1536, 768), (513, 40, 72), (7, 4, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_nn_against_fp64(shape):
    """dx = dy @ W with W (N_out, K_in) read in place"""
    from sigma_amd import gemm
    M, Nout, Kin = shape
    dy, w = _rand(M, Nout, seed=6), _rand(Nout, Kin, seed=7, scale=0.05)
    got = gemm.gemm_nn(dy, w)
    want = dy.double() @ w.double()
    _assert_close(got, want, _bound(dy.double(), w.double()), "nn")


@pytest.mark.parametrize("shape", [(19200, 1536, 384), (19200, 384, 768), (76800, 384, 96), (4800, 96, 192), (300, 1536, 768),
                                   (1001, 68, 36), (33, 4, 4), (31, 128, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_tn_against_fp64(shape):
    """dW = dy^T @ x: reduction over the token dimension, sliced over workgroups, fp32 atomics"""
    from sigma_amd import gemm
    M, Nout, Kin = shape
    dy, x = _rand(M, Nout, seed=8, scale=0.1), _rand(M, Kin, seed=9)
    got = gemm.gemm_tn(dy, x)
    want = dy.double().t() @ x.double()
    _assert_close(got, want, _bound(dy.double().t(), x.double()), "tn")
    acc = torch.ones(Nout, Kin, device=DEV)
    gemm.gemm_tn(dy, x, out=acc, accumulate=True)
    _assert_close(acc, want + 1.0, _bound(dy.double().t(), x.double()) + 1.0, "tn accumulate")


def test_linear_autograd_against_fp64_linear():
    """LinearSplit3Fn: forward, input gradient, weight gradient and bias gradient vs F.linear in fp64."""
    from sigma_amd import gemm
    M, K, N = 2400, 384, 768
    x = _rand(4, M // 4, K, seed=10).requires_grad_()
    w = _rand(N, K, seed=11, scale=0.05).requires_grad_()
    b = _rand(N, seed=12).requires_grad_()
    gy = _rand(4, M // 4, N, seed=13)
    y = gemm.linear(x, w, b)
    y.backward(gy)
    x64, w64, b64 = (t.detach().double().requires_grad_() for t in (x, w, b))
    y64 = torch.nn.functional.linear(x64, w64, b64)
    y64.backward(gy.double())
    for name, got, want in (("y", y, y64), ("dx", x.grad, x64.grad), ("dw", w.grad, w64.grad), ("db", b.grad, b64.grad)):
        rel = float((got.double() - want).abs().max() / want.abs().max())
        assert rel < 5e-5, f"{name}: {rel:.3e}"


def test_gemm_refuses_cpu_tensors_and_bad_shapes():
    from sigma_amd import gemm
    with pytest.raises(RuntimeError):
        gemm.gemm_nt(torch.randn(8, 8), torch.randn(8, 8))
    with pytest.raises(RuntimeError):
        gemm.gemm_nt(_rand(8, 6), _rand(8, 6))                       # K % 4 != 0
    with pytest.raises(RuntimeError):
        gemm.linear(torch.randn(2, 8), torch.randn(4, 8))


# ---- round 4: stacked problems (x_proj / dt_proj of the SS2D core), epilogue addends, outputs shared by problems --------
# (B, d, c, R, L): the four encoder stages of sigma_small at batch 2 (R = dt_rank, c = R + 2 N) and ragged ones
CORE_SHAPES = [(2, 768, 56, 24, 1200), (2, 384, 44, 12, 4800), (1, 1536, 80, 48, 300), (2, 192, 38, 6, 1200), (3, 40, 12, 4, 36)]


@pytest.mark.parametrize("dims", CORE_SHAPES, ids=["x".join(map(str, s)) for s in CORE_SHAPES])
def test_stacked_projections_of_the_scan_core_against_fp64(dims):
    """bgemm_nn with a weight stack shared by groups of problems and strided row-slice operands / outputs (p = W x,
    delta = W_dt p[:R], their input gradients, the last one with the scan's two du as epilogue addends), bgemm_nt_sum
    (weight gradients summed over the batch inside the kernel)."""
    from sigma_amd import gemm
    B, d, c, R, L = dims
    xs = _rand(B, 2, d, L, seed=1)
    Wst = _rand(2, 2 * c, d, seed=2, scale=0.05)
    p4 = torch.empty(B, 4, c, L, device=DEV)
    gemm.bgemm_nn(Wst, xs.view(2 * B, d, L), p4.view(2 * B, 2 * c, L))
    want = torch.matmul(Wst.double().unsqueeze(0), xs.double()).view(B, 4, c, L)
    bound = torch.matmul(Wst.double().abs().unsqueeze(0), xs.double().abs()).view(B, 4, c, L)
    _assert_close(p4, want, bound, "x_proj")
    if R % 4 == 0:
        dtw = _rand(4, d, R, seed=3, scale=0.2)
        delta = torch.full((B, 4, d, L), float("nan"), device=DEV)
        gemm.bgemm_nn(dtw, p4.view(4 * B, c, L)[:, :R], delta.view(4 * B, d, L))
        pr = p4[:, :, :R].double()
        _assert_close(delta, torch.matmul(dtw.double().unsqueeze(0), pr), torch.matmul(dtw.double().abs().unsqueeze(0), pr.abs()), "dt_proj")
        # input gradient of dt_proj written into the first R rows of every group of dp4, the others untouched
        dd = _rand(B, 4, d, L, seed=4)
        dp4 = torch.full((B, 4, c, L), 7.0, device=DEV)
        gemm.bgemm_nn(dtw.transpose(1, 2).contiguous(), dd.view(4 * B, d, L), dp4.view(4 * B, c, L)[:, :R])
        wt = dtw.double().transpose(1, 2).unsqueeze(0)
        _assert_close(dp4[:, :, :R], torch.matmul(wt, dd.double()), torch.matmul(wt.abs(), dd.double().abs()), "dt_proj dgrad")
        assert bool((dp4[:, :, R:] == 7.0).all())
        # weight gradient summed over the batch
        dW = torch.zeros(4, d, R, device=DEV)
        gemm.bgemm_nt_sum(dd.view(4 * B, d, L), p4.view(4 * B, c, L)[:, :R], dW)
        wantW = torch.matmul(dd.double(), pr.transpose(-1, -2)).sum(0)
        boundW = torch.matmul(dd.double().abs(), pr.abs().transpose(-1, -2)).sum(0)
        _assert_close(dW, wantW, boundW, "dt_proj wgrad")
    # x_proj input gradient + the scan's du of both directions of an order, one pass
    dp = _rand(B, 4, c, L, seed=5)
    du = _rand(B, 4, d, L, seed=6)
    du3 = du.view(2 * B, 2, d, L)
    dxs = torch.empty(B, 2, d, L, device=DEV)
    gemm.bgemm_nn(Wst.transpose(1, 2).contiguous(), dp.view(2 * B, 2 * c, L), dxs.view(2 * B, d, L), residual=du3[:, 0], residual2=du3[:, 1])
    wt = Wst.double().transpose(1, 2).unsqueeze(0)
    dp2 = dp.double().view(B, 2, 2 * c, L)
    want = torch.matmul(wt, dp2) + du.double().view(B, 2, 2, d, L).sum(2)
    bound = torch.matmul(wt.abs(), dp2.abs()) + du.double().abs().view(B, 2, 2, d, L).sum(2)
    _assert_close(dxs, want, bound, "x_proj dgrad + du")
    dWst = torch.zeros(2, 2 * c, d, device=DEV)
    gemm.bgemm_nt_sum(dp.view(2 * B, 2 * c, L), xs.view(2 * B, d, L), dWst)
    wantW = torch.matmul(dp2, xs.double().transpose(-1, -2)).sum(0)
    boundW = torch.matmul(dp2.abs(), xs.double().abs().transpose(-1, -2)).sum(0)
    _assert_close(dWst, wantW, boundW, "x_proj wgrad")


@pytest.mark.parametrize("shape", [(19200, 768, 384), (4800, 384, 192), (257, 100, 72), (130, 36, 200), (5, 4, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_linear_with_the_residual_added_in_the_kernel(shape):
    """y = x W^T (+ b) + r with r entering through the accumulators: value, and the gradients of x, W, b and r"""
    from sigma_amd import gemm
    M, K, N = shape
    x, w, b, r = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=0.05), _rand(N, seed=3), _rand(M, N, seed=4)
    for bias in (None, b):
        y = gemm.gemm_nt(x, w, bias, residual=r)
        want = x.double() @ w.double().t() + r.double() + (0 if bias is None else bias.double())
        _assert_close(y, want, _bound(x.double(), w.double().t()) + r.double().abs() + 1.0, "nt + residual")
    xa, wa, ba, ra = (t.clone().requires_grad_() for t in (x, w, b, r))
    g = _rand(M, N, seed=5)
    gemm.linear(xa.view(1, M, K), wa, ba, residual=ra.view(1, M, N)).backward(g.view(1, M, N))
    xr, wr, br, rr = (t.double().clone().requires_grad_() for t in (x, w, b, r))
    (torch.nn.functional.linear(xr, wr, br) + rr).backward(g.double())
    assert torch.equal(ra.grad, g)
    torch.testing.assert_close(ba.grad.double(), br.grad, rtol=1e-4, atol=1e-3)
    _assert_close(xa.grad, xr.grad, _bound(g.double().abs(), w.double().abs()), "dx")
    _assert_close(wa.grad, wr.grad, _bound(g.double().t().abs(), x.double().abs()), "dW")


def test_stacked_gemms_refuse_what_they_cannot_take():
    from sigma_amd import gemm
    a, b, o = _rand(2, 8, 16), _rand(4, 16, 24), torch.empty(4, 8, 24, device=DEV)
    gemm.bgemm_nn(a, b, o)
    with pytest.raises(RuntimeError):
        gemm.bgemm_nn(_rand(3, 8, 16), b, o)                       # 3 does not divide 4
    with pytest.raises(RuntimeError):
        gemm.bgemm_nn(a, _rand(4, 16, 22), torch.empty(4, 8, 22, device=DEV))     # N % 4
    with pytest.raises(RuntimeError):
        gemm.bgemm_nn(a.cpu(), b.cpu(), o.cpu())
    with pytest.raises(RuntimeError):
        gemm.bgemm_nn(a, b, o, residual2=o)
    with pytest.raises(RuntimeError):
        gemm.bgemm_nt_sum(_rand(4, 8, 16), _rand(4, 24, 16), torch.zeros(3, 8, 24, device=DEV))
    with pytest.raises(RuntimeError):
        gemm.gemm_nt(_rand(8, 16), _rand(24, 16), residual=_rand(8, 20))


# ---- round 6: in_proj with a channel-major x half (sigma_gemm.h t_cols), sliced reductions of the nn form ------------------

XZ_SHAPES = [(2, 30, 40, 384, 768), (2, 6, 10, 96, 192), (1, 15, 20, 768, 1536), (2, 23, 40, 128, 256), (1, 3, 4, 32, 32)]


@pytest.mark.parametrize("dims", XZ_SHAPES, ids=["x".join(map(str, d)) for d in XZ_SHAPES])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_in_proj_with_channel_major_x_half_against_fp64(dims, with_bias):
    """gemm.linear_xz (vmamba.py:1067-1071: in_proj, chunk, permute + contiguous of the x half): ONE GEMM whose x columns
    leave the kernel transposed.  Forward and the gradients of x, weight and bias against the fp64 formulation; the x half is
    a (B, d, H, W) view of a channel-major (d, B, H, W) buffer whose planes are contiguous."""
    from sigma_amd import gemm
    B, H, W, C, d = dims
    x = _rand(B, H, W, C, seed=31).requires_grad_()
    w = _rand(2 * d, C, seed=32, scale=0.05).requires_grad_()
    b = _rand(2 * d, seed=33, scale=0.1).requires_grad_() if with_bias else None
    assert gemm.xz_ok(x.reshape(-1, C), w)
    xi, z = gemm.linear_xz(x, w, b)
    assert tuple(xi.shape) == (B, d, H, W) and xi.stride()[2:] == (W, 1) and xi.stride(1) == B * H * W and z.is_contiguous()
    x64, w64 = x.detach().double().requires_grad_(), w.detach().double().requires_grad_()
    b64 = b.detach().double().requires_grad_() if with_bias else None
    ref = torch.nn.functional.linear(x64, w64, b64)
    bound = _bound(x64.detach().reshape(-1, C), w64.detach().t())
    _assert_close(xi.permute(0, 2, 3, 1).reshape(-1, d), ref[..., :d].reshape(-1, d).detach(), bound[:, :d], "x half")
    _assert_close(z.reshape(-1, d), ref[..., d:].reshape(-1, d).detach(), bound[:, d:], "z half")
    gx, gz = _rand(*xi.shape, seed=34), _rand(*z.shape, seed=35)
    ((xi * gx).sum() + (z * gz).sum()).backward()
    ((ref[..., :d].permute(0, 3, 1, 2) * gx.double()).sum() + (ref[..., d:] * gz.double()).sum()).backward()
    g2 = torch.cat([gx.permute(0, 2, 3, 1).reshape(-1, d), gz.reshape(-1, d)], 1).double()
    _assert_close(x.grad.reshape(-1, C), x64.grad.reshape(-1, C), _bound(g2, w64.detach()), "dx")
    _assert_close(w.grad, w64.grad, _bound(g2.t(), x64.detach().reshape(-1, C)), "dw")
    if with_bias:
        torch.testing.assert_close(b.grad.double(), b64.grad, rtol=1e-4, atol=1e-4 * float(b64.grad.abs().max()))


def test_transposed_column_range_refuses_what_it_cannot_take():
    """t_cols needs 32-column granularity, M % 4 == 0, plain stores (no accumulate / residual): SIGMA_OPS_ERR_ARG otherwise"""
    from sigma_amd import gemm
    a, w = _rand(64, 32, seed=1), _rand(128, 32, seed=2)
    z, xt = torch.empty(64, 64, device=DEV), torch.empty(64, 64, device=DEV)
    ok = gemm._params(64, 128, 32, a, w, z, None, 32, 32, 64, out_t=xt, ldct=64, t_cols=64)
    gemm._run("sigma_gemm_nt_split3", ok, a.device)                                  # the legal call
    want = a.double() @ w.double().t()
    _assert_close(xt.t(), want[:, :64], _bound(a.double(), w.double().t())[:, :64], "transposed half")
    _assert_close(z, want[:, 64:], _bound(a.double(), w.double().t())[:, 64:], "plain half")
    for kw in (dict(t_cols=48), dict(t_cols=160), dict(ldct=60), dict(accumulate=True)):
        args = dict(out_t=xt, ldct=64, t_cols=64)
        acc = kw.pop("accumulate", False)
        args.update(kw)
        p = gemm._params(64, 128, 32, a, w, z, None, 32, 32, 64, acc, **args)
        with pytest.raises(RuntimeError, match="sigma_gemm_nt_split3 failed"):
            gemm._run("sigma_gemm_nt_split3", p, a.device)
    a2 = _rand(66, 32, seed=3)                                                        # M % 4 != 0
    p = gemm._params(66, 128, 32, a2, w, torch.empty(66, 64, device=DEV), None, 32, 32, 64, out_t=torch.empty(64, 68, device=DEV), ldct=68, t_cols=64)
    with pytest.raises(RuntimeError, match="sigma_gemm_nt_split3 failed"):
        gemm._run("sigma_gemm_nt_split3", p, a.device)


@pytest.mark.parametrize("shape", [(768, 19200, 384), (192, 4800, 96), (1536, 300, 768), (64, 4096, 32), (130, 1000, 36)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_nn_with_a_sliced_reduction_against_fp64(shape):
    """k_slices: few output tiles, a long reduction (dW_x = dx^T x with dx held channel-major): slices summed with atomics
    into a zero-filled output; also into a row-slice view of a larger gradient tensor, and accumulating"""
    from sigma_amd import gemm
    M, K, N = shape
    a, b = _rand(M, K, seed=41), _rand(K, N, seed=42, scale=0.05)
    want = a.double() @ b.double()
    bound = _bound(a.double(), b.double())
    _assert_close(gemm.gemm_nn(a, b, k_slices=True), want, bound, "nn sliced")
    big = torch.full((2 * M, N), 7.0, device=DEV)
    gemm.gemm_nn(a, b, out=big[M:], k_slices=True)
    _assert_close(big[M:], want, bound, "nn sliced into a view")
    assert float((big[:M] - 7.0).abs().max()) == 0.0
    acc = _rand(M, N, seed=43)
    got = gemm.gemm_nn(a, b, out=acc.clone(), accumulate=True, k_slices=True)
    _assert_close(got, want + acc.double(), bound + acc.double().abs(), "nn sliced accumulate")


@pytest.mark.parametrize("shape", [(19200, 1536, 384), (19200, 384, 768), (4800, 96, 192), (1001, 68, 36)],
                         ids=lambda s: "x".join(map(str, s)))
def test_sliced_reductions_sum_in_two_stages_without_a_zero_fill(shape):
    """Round 6: the reduction slices of a weight gradient are stored as partial results in scratch and summed by a second
    kernel (sigma_gemm_workspace_bytes / params.workspace): the output needs no zero fill (here it holds NaN), two runs
    agree bit for bit, `accumulate` adds, and a caller WITHOUT scratch still gets the atomic sums into a zero-filled C."""
    import ctypes
    from sigma_amd import _capi, gemm
    M, Nout, Kin = shape
    dy, x = _rand(M, Nout, seed=8, scale=0.1), _rand(M, Kin, seed=9)
    want = dy.double().t() @ x.double()
    bound = _bound(dy.double().t(), x.double())
    out = torch.full((Nout, Kin), float("nan"), device=DEV)
    gemm.gemm_tn(dy, x, out=out)
    _assert_close(out, want, bound, "tn into NaN")
    again = torch.full((Nout, Kin), float("nan"), device=DEV)
    gemm.gemm_tn(dy, x, out=again)
    assert torch.equal(out, again)                              # fixed summation order
    big = torch.full((2 * Nout, Kin), 3.0, device=DEV)          # a row-slice view of a larger gradient tensor
    gemm.gemm_tn(dy, x, out=big[Nout:])
    assert torch.equal(big[Nout:], out) and float((big[:Nout] - 3.0).abs().max()) == 0.0
    # the C ABI without scratch: atomics into a zero-filled C
    p = gemm._params(M, Nout, Kin, dy, x, out, None, dy.stride(0), x.stride(0), out.stride(0), False)
    need = int(_capi.load().sigma_gemm_workspace_bytes(ctypes.byref(p), 2))
    assert need >= 0
    out.zero_()
    with torch.cuda.device(dy.device):
        rc = _capi.load().sigma_gemm_tn_split3(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    _assert_close(out, want, bound, "tn atomics")
    if need > 0:                                                 # scratch one byte short: refused as scratch, atomics again
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        p.workspace, p.workspace_bytes = ws.data_ptr(), need - 1
        out.zero_()
        with torch.cuda.device(dy.device):
            assert _capi.load().sigma_gemm_tn_split3(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        _assert_close(out, want, bound, "tn short scratch")
        p.workspace, p.workspace_bytes = None, 16                # bytes without a pointer
        with torch.cuda.device(dy.device):
            assert _capi.load().sigma_gemm_tn_split3(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0


def test_shared_outputs_sum_in_two_stages():
    """bgemm_nt_sum (weight gradients of the stacked projections summed over the batch): overwrite into NaN, accumulate,
    bit-identical repeats (ragged problem counts per output: test_ragged_shared_outputs_follow_the_workspace_contract)"""
    from sigma_amd import gemm
    B, d, c, L = 8, 192, 16, 1200
    dp, xs = _rand(2 * B, 2 * c, L, seed=51), _rand(2 * B, d, L, seed=52)
    want = torch.matmul(dp.double(), xs.double().transpose(-1, -2)).view(B, 2, 2 * c, d).sum(0)
    bound = torch.matmul(dp.double().abs(), xs.double().abs().transpose(-1, -2)).view(B, 2, 2 * c, d).sum(0)
    out = torch.full((2, 2 * c, d), float("nan"), device=DEV)
    gemm.bgemm_nt_sum(dp, xs, out, accumulate=False)
    _assert_close(out, want, bound, "nt_sum overwrite")
    again = torch.full((2, 2 * c, d), float("nan"), device=DEV)
    gemm.bgemm_nt_sum(dp, xs, again, accumulate=False)
    assert torch.equal(out, again)
    acc = torch.ones(2, 2 * c, d, device=DEV)
    gemm.bgemm_nt_sum(dp, xs, acc)
    _assert_close(acc, want + 1.0, bound + 1.0, "nt_sum accumulate")


# guard bands: shared with the exact suite (tests/gemm_exact_ref.py)
from tests.gemm_exact_ref import guarded as _guarded, margins_intact as _margins_intact  # noqa: E402


def _call(name, p, dev):
    import ctypes
    from sigma_amd import _capi
    with torch.cuda.device(dev):
        return int(getattr(_capi.load(), name)(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def test_ragged_shared_outputs_follow_the_workspace_contract():
    """c_mod with batch % c_mod != 0 (5 problems into 2 outputs: output 0 sums z = 0, 2, 4, output 1 sums z = 1, 3), called
    exactly as include/sigma_gemm.h says: query the scratch, pass what it asks for, accumulate = 0, no zero fill (C holds
    NaN).  The query used to answer 0 ("no scratch needed") for ragged groups and the launch then added fp32 atomics onto
    the uninitialised C.  Same bound as the other nt cases; the guard bands around C stay NaN."""
    import ctypes
    from sigma_amd import _capi, gemm
    Z, cm, M, N, K = 5, 2, 32, 192, 1200
    a, b = _rand(Z, M, K, seed=61), _rand(Z, N, K, seed=62, scale=0.05)
    margin = N + 64
    buf, flat = _guarded(cm * M * N, margin)
    c = flat.view(cm, M, N)
    p = gemm._params(M, N, K, a, b, c, None, K, K, N, False, batch=Z, sA=M * K, sB=N * K, sC=M * N, c_mod=cm)
    need = int(_capi.load().sigma_gemm_workspace_bytes(ctypes.byref(p), 0))
    assert need > 0, "a shared-output launch must ask for the scratch of its two-stage sum"
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    p.workspace, p.workspace_bytes = ws.data_ptr(), need
    gemm._selftest(a.device)
    assert _call("sigma_gemm_nt_split3", p, a.device) == 0
    prod = torch.matmul(a.double(), b.double().transpose(-1, -2))
    absp = torch.matmul(a.double().abs(), b.double().abs().transpose(-1, -2))
    want = torch.stack([prod[0::2].sum(0), prod[1::2].sum(0)])
    bound = torch.stack([absp[0::2].sum(0), absp[1::2].sum(0)])
    assert _margins_intact(buf, cm * M * N, margin), "ragged c_mod wrote outside C"
    _assert_close(c, want, bound, "ragged c_mod")
    # accumulate = 1 through the same scratch adds to what C holds
    c.copy_(torch.ones_like(c))
    p.accumulate = 1
    assert _call("sigma_gemm_nt_split3", p, a.device) == 0
    _assert_close(c, want + 1.0, bound + 1.0, "ragged c_mod accumulate")
    assert _margins_intact(buf, cm * M * N, margin)


def test_transposed_column_range_ignores_the_batch_stride_of_a_single_problem():
    """t_cols = 32 with batch = 1 and strideC = 2: a single problem never steps by strideC, but a stride that was not a
    multiple of 4 used to switch the kernel to its direct epilogue, which knows no t_cols -- it wrote all N columns into
    the (N - t_cols)-wide C (past its end) and none into Ct.  Both outputs sit inside NaN guard bands."""
    from sigma_amd import gemm
    M, N, K, T = 64, 128, 32, 32
    a, w = _rand(M, K, seed=71), _rand(N, K, seed=72)
    mc, mt = (N - T) + 64, M + 64
    cbuf, cflat = _guarded(M * (N - T), mc)
    tbuf, tflat = _guarded(T * M, mt)
    c, ct = cflat.view(M, N - T), tflat.view(T, M)
    p = gemm._params(M, N, K, a, w, c, None, K, K, N - T, sC=2, out_t=ct, ldct=M, t_cols=T)
    gemm._selftest(a.device)
    assert _call("sigma_gemm_nt_split3", p, a.device) == 0
    assert _margins_intact(cbuf, M * (N - T), mc), "C overrun"
    assert _margins_intact(tbuf, T * M, mt), "Ct overrun"
    want = a.double() @ w.double().t()
    bound = _bound(a.double(), w.double().t())
    _assert_close(ct.t(), want[:, :T], bound[:, :T], "transposed columns")
    _assert_close(c, want[:, T:], bound[:, T:], "plain columns")


@pytest.mark.parametrize("c_mod", [0, 2, 4])
def test_sliced_nn_of_one_problem_ignores_a_larger_c_mod(c_mod):
    """nn with k_slices, batch = 1 and c_mod >= 2 (legal: c_mod >= batch means no output is shared): the two-stage sum of
    the slices must cover the one output that exists -- scratch sized for c_mod outputs made the reduce kernel write a
    zero (or race with the real sum) for outputs no problem owns.  Called by the header's contract into a NaN guard band:
    query, the scratch it asks for, accumulate = 0."""
    import ctypes
    from sigma_amd import _capi, gemm
    M, N, K = 64, 64, 19200
    a, b = _rand(M, K, seed=81), _rand(K, N, seed=82, scale=0.05)
    margin = N + 64
    buf, flat = _guarded(M * N, margin)
    c = flat.view(M, N)
    p = gemm._params(M, N, K, a, b, c, None, K, N, N, False, sC=M * N, c_mod=c_mod, k_slices=1)
    need = int(_capi.load().sigma_gemm_workspace_bytes(ctypes.byref(p), 1))
    assert need > 0 and need % (M * N * 4) == 0
    ws = torch.full((need // 4,), float("nan"), device=DEV)
    p.workspace, p.workspace_bytes = ws.data_ptr(), need
    gemm._selftest(a.device)
    assert _call("sigma_gemm_nn_split3", p, a.device) == 0
    assert _margins_intact(buf, M * N, margin), "sliced nn wrote outside C"
    want = a.double() @ b.double()
    _assert_close(c, want, _bound(a.double(), b.double()), f"sliced nn, c_mod {c_mod}")
    first = c.clone()
    assert _call("sigma_gemm_nn_split3", p, a.device) == 0
    assert torch.equal(c, first)                                  # fixed summation order, no racing stores


# ---- operands scaled per row and per column over 2^-40 .. 2^40 -----------------------------------------------------------

def _pow2_scales(n, seed, lo=-40, hi=40):
    """n powers of two with exponents spread evenly over [lo, hi], in a shuffled order"""
    g = torch.Generator().manual_seed(seed)
    e = torch.linspace(lo, hi, n).round()[torch.randperm(n, generator=g)]
    return torch.pow(2.0, e).to(DEV)


@pytest.mark.parametrize("form", ["nt", "nn", "tn"])
def test_gemm_keeps_its_relative_bound_under_row_and_column_scales(form):
    """C = diag(r) (A B) diag(c) with r, c powers of two from 2^-40 to 2^40: bf16 keeps fp32's exponent, so every piece,
    product and sum scales exactly and the error bound relative to sum |a||b| must hold UNCHANGED (outputs range over
    2^-80 .. 2^80; products and lo pieces stay normal in bf16 and fp32).  A scale shared by a tile, a narrower
    accumulator or a piece held in fp16 anywhere would break it.  nt, nn, and tn with reduction slices."""
    from sigma_amd import gemm
    M, N, K = (8000, 132, 200) if form == "tn" else (300, 200, 132)          # tn: C is N x K, 8000 tokens in several slices
    rows, cols = (N, K) if form == "tn" else (M, N)
    r, c = _pow2_scales(rows, 91), _pow2_scales(cols, 92)
    if form == "nt":
        a, b = _rand(M, K, seed=93) * r[:, None], _rand(N, K, seed=94, scale=0.05) * c[:, None]
        got, a64, b64 = gemm.gemm_nt(a, b), a.double(), b.double().t()
    elif form == "nn":
        a, b = _rand(M, K, seed=93) * r[:, None], _rand(K, N, seed=94, scale=0.05) * c[None, :]
        got, a64, b64 = gemm.gemm_nn(a, b), a.double(), b.double()
    else:
        a, b = _rand(M, N, seed=93, scale=0.1) * r[None, :], _rand(M, K, seed=94) * c[None, :]
        got, a64, b64 = gemm.gemm_tn(a, b), a.double().t(), b.double()
    want, bound = a64 @ b64, _bound(a64, b64)
    assert float(bound.min()) > 2.0 ** -110 and float(bound.max()) < 2.0 ** 100 and bool(torch.isfinite(got).all())
    err = (got.double() - want).abs()
    worst = float((err / bound).max())
    assert worst < 3e-5, f"{form} scaled: max error / sum|a||b| = {worst:.3e}"
    # the rms check of _assert_close per output element's own scale (a global rms would only see the largest scales)
    rel = err / (r[:, None].double() * c[None, :].double())
    ref = want / (r[:, None].double() * c[None, :].double())
    rms = float(rel.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    assert rms < 2e-5, f"{form} scaled: relative rms error {rms:.3e}"


# ---- non-finite operand elements, the bf16 overflow edge, small magnitudes ------------------------------------------------
# Non-finite VALUES are data, not addresses: no test here makes a kernel read or write outside memory the test owns.
# Contract (include/sigma_gemm.h): split_pair turns an operand element of +-inf, or a finite one whose magnitude rounds to
# inf in bf16 (bit pattern 0x7F7F8000 and above), into the pieces (inf, NaN) / (inf, -inf): its row (A) or column (B) of C
# is NaN where an fp32 GEMM returns +-inf or stays finite -- and nothing else of C moves.

NONFINITE = (float("nan"), float("inf"), float("-inf"))
REPORT: dict = {}


def _from_bits(bits):
    return torch.tensor([bits], dtype=torch.int32).view(torch.float32).item()


def _same_or_bound(got, clean, want64, bound, keep, what):
    """outside the footprint: bit-identical to the unplanted run where the launch sums in a fixed order (two-stage /
    deterministic mode, and launches whose work items own their outputs), inside the existing bound otherwise"""
    from sigma_amd import gemm
    assert bool(torch.isfinite(got[keep]).all()), f"{what}: non-finite outside the footprint"
    if gemm._two_stage():
        assert torch.equal(got[keep], clean[keep]), f"{what}: {int((got[keep] != clean[keep]).sum())} elements outside the footprint moved"
    else:
        err = (got.double() - want64).abs()[keep]
        assert float((err / (bound[keep] + 1e-30)).max()) < 3e-5, what


def _footprint_of(form_mm, a, b, who, idx):
    """set arithmetic: the elements of C that have the planted element among their terms"""
    ma, mb = torch.zeros_like(a, dtype=torch.float64), torch.zeros_like(b, dtype=torch.float64)
    (ma if who == "a" else mb)[idx] = 1.0
    return (form_mm(ma, torch.ones_like(mb)) + form_mm(torch.ones_like(ma), mb)) > 0


def _check_plants(run, form_mm, a, b, plants, what, nan_only=True):
    """``run(a, b)`` -> C.  For every plant (operand, index) and every value of NONFINITE: C is NaN exactly on the
    footprint of the plant, everything else as in the unplanted run"""
    clean = run(a, b).clone()
    want64, bound = form_mm(a.double(), b.double()), form_mm(a.double().abs(), b.double().abs())
    assert bool(torch.isfinite(clean).all())
    for who, idx in plants:
        for v in NONFINITE:
            pa, pb = a.clone(), b.clone()
            (pa if who == "a" else pb)[idx] = v
            got = run(pa, pb)
            cone = _footprint_of(form_mm, a, b, who, idx)
            assert bool(cone.any()) and not bool(cone.all()), (what, who, idx)
            bad = torch.isnan(got) if nan_only else ~torch.isfinite(got)
            assert bool(bad[cone].all()), f"{what} {who}{idx} = {v}: {int((~bad[cone]).sum())} elements of the footprint are not NaN"
            _same_or_bound(got, clean, want64, bound, ~cone, f"{what} {who}{idx} = {v}")


def _ab_plants(a_shape, b_shape, a_rk, b_ck):
    """one plant in the full part and one in each partial part: (row, k) of A and (column, k) of B given as axis numbers"""
    out = []
    for who, shape, (ax, kx) in (("a", a_shape, a_rk), ("b", b_shape, b_ck)):
        for r, k in ((5, 3), (shape[ax] - 1, shape[kx] - 1)):
            idx = [0] * len(shape)
            idx[ax], idx[kx] = r, k
            out.append((who, tuple(idx)))
    return out


# (M, K, N): a partial row tile, a partial column tile and a partial last k-step (K % 32 != 0)
FOOT_SHAPES = [(130, 36, 200), (257, 100, 72)]


@pytest.mark.parametrize("pieces", [2, 3])
@pytest.mark.parametrize("shape", FOOT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", ["nt", "nn", "tn"])
def test_one_non_finite_operand_element_reaches_its_row_or_column_only(form, shape, pieces):
    """NaN, +inf and -inf in one element of A and of B, in the full and in the partial tiles / k-step: C is NaN exactly on
    that row (A) or column (B) -- +-inf too: the pieces of inf are (inf, NaN) -- and bit-identical elsewhere"""
    from sigma_amd import gemm
    M, K, N = shape
    if form == "nt":
        a, b = _rand(M, K, seed=101), _rand(N, K, seed=102, scale=0.05)
        run, mm, plants = (lambda x, y: gemm.gemm_nt(x, y, pieces=pieces)), (lambda x, y: x @ y.t()), _ab_plants(a.shape, b.shape, (0, 1), (0, 1))
    elif form == "nn":
        a, b = _rand(M, K, seed=101), _rand(K, N, seed=102, scale=0.05)
        run, mm, plants = (lambda x, y: gemm.gemm_nn(x, y, pieces=pieces)), (lambda x, y: x @ y), _ab_plants(a.shape, b.shape, (0, 1), (1, 0))
    else:                                                    # reduction over the K tokens, C is M x N (M a multiple of 4)
        M = (M + 3) // 4 * 4
        a, b = _rand(K, M, seed=101, scale=0.1), _rand(K, N, seed=102)
        run, mm, plants = (lambda x, y: gemm.gemm_tn(x, y, pieces=pieces)), (lambda x, y: x.t() @ y), _ab_plants(a.shape, b.shape, (1, 0), (1, 0))
    _check_plants(run, mm, a, b, plants, f"{form} p{pieces}")


def test_non_finite_elements_in_a_sliced_tn_stay_in_their_row_or_column():
    """tn with several reduction slices summed in two stages (8004 tokens, 8004 % 32 = 4): a plant in the first slice, one in
    the last, partial k-step -- the row / column of C is NaN, the rest bit-identical"""
    from sigma_amd import gemm
    T, N, K = 8004, 132, 200
    a, b = _rand(T, N, seed=103, scale=0.1), _rand(T, K, seed=104)
    out = lambda x, y: gemm.gemm_tn(x, y, out=torch.full((N, K), float("nan"), device=DEV))
    plants = [("a", (3, 5)), ("a", (T - 1, N - 1)), ("b", (4000, 7)), ("b", (T - 1, K - 1))]
    _check_plants(out, lambda x, y: x.t() @ y, a, b, plants, "tn sliced")


def test_non_finite_bias_and_addends_reach_their_column_or_element_only():
    """nt with bias and a residual; bgemm_nn with both epilogue addends: a plant in the bias makes its column non-finite
    (+-inf stays +-inf: the epilogue adds in fp32), a plant in an addend its one element"""
    from sigma_amd import gemm
    M, K, N = 130, 36, 200
    x, w, bias, r = _rand(M, K, seed=105), _rand(N, K, seed=106, scale=0.05), _rand(N, seed=107), _rand(M, N, seed=108)
    clean = gemm.gemm_nt(x, w, bias, residual=r).clone()
    for v in NONFINITE:
        for j in (7, N - 1):
            pb = bias.clone()
            pb[j] = v
            got = gemm.gemm_nt(x, w, pb, residual=r)
            keep = torch.ones_like(got, dtype=torch.bool)
            keep[:, j] = False
            assert not bool(torch.isfinite(got[:, j]).any()) and torch.equal(got[keep], clean[keep]), ("bias", j, v)
        for i, j in ((5, 7), (M - 1, N - 1), (M - 1, 3), (2, N - 1)):
            pr = r.clone()
            pr[i, j] = v
            got = gemm.gemm_nt(x, w, bias, residual=pr)
            keep = torch.ones_like(got, dtype=torch.bool)
            keep[i, j] = False
            assert not bool(torch.isfinite(got[i, j])) and torch.equal(got[keep], clean[keep]), ("residual", i, j, v)
    Z, c2, d, L = 4, 36, 132, 200                           # the stacked x_proj input gradient + the scan's two du
    Wt, dp = _rand(2, d, c2, seed=109, scale=0.05), _rand(Z, c2, L, seed=110)
    du = _rand(Z, 2, d, L, seed=111)
    run = lambda r1, r2: gemm.bgemm_nn(Wt, dp, torch.empty(Z, d, L, device=DEV), residual=r1, residual2=r2)
    clean = run(du[:, 0], du[:, 1]).clone()
    for v in NONFINITE:
        for which in (0, 1):
            for z, i, j in ((1, 5, 7), (Z - 1, d - 1, L - 1)):
                pd = du.clone()
                pd[z, which, i, j] = v
                got = run(pd[:, 0], pd[:, 1])
                keep = torch.ones_like(got, dtype=torch.bool)
                keep[z, i, j] = False
                assert not bool(torch.isfinite(got[z, i, j])) and torch.equal(got[keep], clean[keep]), ("addend", which, z, i, j, v)


def test_non_finite_elements_of_shared_weights_and_shared_outputs():
    """bgemm_nn with a weight stack shared by problems (a_mod): a plant in the weight reaches its row of EVERY problem
    that reads it, a plant in a problem's own operand its column of that problem.  Outputs shared by problems (c_mod):
    exactly the shared output that the planted problem adds into, even (bgemm_nt_sum, 4 problems on 2 outputs) and ragged
    (5 problems on 2 outputs, through the C ABI by the header's contract)."""
    import ctypes
    from sigma_amd import _capi, gemm
    Z, am, M, K, N = 4, 2, 72, 36, 200
    W, X = _rand(am, M, K, seed=112, scale=0.05), _rand(Z, K, N, seed=113)
    run = lambda w, x: gemm.bgemm_nn(w, x, torch.empty(Z, M, N, device=DEV))
    mm = lambda w, x: torch.matmul(w[torch.arange(Z, device=w.device) % am], x)
    _check_plants(run, mm, W, X, [("a", (1, 5, 3)), ("a", (0, M - 1, K - 1)), ("b", (2, 3, 7)), ("b", (Z - 1, K - 1, N - 1))], "bgemm_nn a_mod")

    def fold(p, cm):                                         # problems z with the same z % cm summed
        out = torch.zeros((cm,) + tuple(p.shape[1:]), dtype=p.dtype, device=p.device)
        return out.index_add_(0, torch.arange(p.shape[0], device=p.device) % cm, p)

    Z, cm, M, N, K = 4, 2, 40, 132, 200
    a, b = _rand(Z, M, K, seed=114), _rand(Z, N, K, seed=115, scale=0.05)
    run = lambda x, y: gemm.bgemm_nt_sum(x, y, torch.full((cm, M, N), float("nan"), device=DEV), accumulate=False)
    mm = lambda x, y: fold(torch.matmul(x, y.transpose(-1, -2)), cm)
    _check_plants(run, mm, a, b, [("a", (0, 5, 3)), ("a", (3, M - 1, K - 1)), ("b", (1, 7, 3)), ("b", (2, N - 1, K - 1))], "c_mod even")

    Z, cm, M, N, K = 5, 2, 32, 192, 1204                    # ragged: output 0 sums z = 0, 2, 4, output 1 sums z = 1, 3
    a, b = _rand(Z, M, K, seed=116), _rand(Z, N, K, seed=117, scale=0.05)

    def ragged(x, y):
        margin = N + 64
        buf, flat = _guarded(cm * M * N, margin)
        c = flat.view(cm, M, N)
        p = gemm._params(M, N, K, x, y, c, None, K, K, N, False, batch=Z, sA=M * K, sB=N * K, sC=M * N, c_mod=cm)
        need = int(_capi.load().sigma_gemm_workspace_bytes(ctypes.byref(p), 0))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        p.workspace, p.workspace_bytes = ws.data_ptr(), need
        gemm._selftest(x.device)
        assert _call("sigma_gemm_nt_split3", p, x.device) == 0
        assert _margins_intact(buf, cm * M * N, margin), "ragged c_mod wrote outside C"
        return c

    mm = lambda x, y: fold(torch.matmul(x, y.transpose(-1, -2)), cm)
    _check_plants(ragged, mm, a, b, [("a", (4, 5, 3)), ("a", (3, M - 1, K - 1)), ("b", (2, 7, 1203)), ("b", (0, N - 1, 40))], "c_mod ragged")


def test_non_finite_elements_with_a_transposed_column_range():
    """in_proj with the x half leaving the kernel transposed (t_cols): 132 tokens, K = 36, 96 + 96 columns -- a plant in a
    token reaches that token in BOTH halves, a plant in a weight row its one column, in whichever half it lies"""
    from sigma_amd import gemm
    Bn, H, W_, C, d = 1, 3, 44, 36, 96
    x, w = _rand(Bn * H * W_, C, seed=118), _rand(2 * d, C, seed=119, scale=0.05)
    assert gemm.xz_ok(x, w)

    def run(xx, ww):
        with torch.no_grad():
            xi, z = gemm.linear_xz(xx.view(Bn, H, W_, C), ww, None)
        return torch.cat([xi.permute(0, 2, 3, 1).reshape(-1, d), z.reshape(-1, d)], 1)

    plants = [("a", (5, 3)), ("a", (131, 35)), ("b", (7, 3)), ("b", (d - 1, 35)), ("b", (d, 0)), ("b", (2 * d - 1, 35))]
    _check_plants(run, lambda a_, b_: a_ @ b_.t(), x, w, plants, "t_cols")


def test_bf16_overflow_edge_of_the_split_is_pinned():
    """the contract difference from an fp32 GEMM: an operand element whose magnitude rounds to inf in bf16 -- bit pattern
    0x7F7F8000 (about 3.396e38, finite in fp32) and above -- splits into (inf, -inf) and makes its row or column of C NaN,
    and only that; 0x7F7F7FFF, the largest safe one, splits into finite pieces and keeps the usual bound.  B is scaled by
    2^-30 so that the fp32 result itself stays finite."""
    from sigma_amd import gemm
    M, K, N = 130, 36, 200
    a, w = _rand(M, K, seed=120), _rand(N, K, seed=121, scale=0.05 * 2.0 ** -30)
    clean = gemm.gemm_nt(a, w).clone()
    safe, unsafe = _from_bits(0x7F7F7FFF), _from_bits(0x7F7F8000)
    assert safe < unsafe < float("inf")
    for sign in (1.0, -1.0):
        for who, idx in (("a", (5, 3)), ("a", (M - 1, K - 1)), ("b", (7, 3)), ("b", (N - 1, K - 1))):
            pa, pw = a.clone(), w.clone()
            (pa if who == "a" else pw)[idx] = sign * unsafe
            got = gemm.gemm_nt(pa, pw)
            cone = _footprint_of(lambda x, y: x @ y.t(), a, w, who, idx)
            assert bool(torch.isnan(got[cone]).all()), (who, idx, "an element above the bf16 threshold must give NaN")
            assert torch.equal(got[~cone], clean[~cone]), (who, idx)
        pa = a.clone()
        pa[5, 3] = sign * safe
        got = gemm.gemm_nt(pa, w)
        want = pa.double() @ w.double().t()
        assert bool(torch.isfinite(got).all())
        _assert_close(got[5:6], want[5:6], _bound(pa.double(), w.double().t())[5:6], "largest safe magnitude")
        assert torch.equal(torch.cat([got[:5], got[6:]]), torch.cat([clean[:5], clean[6:]]))


@pytest.mark.parametrize("form", ["nt", "nn", "tn"])
def test_gemm_bound_on_small_magnitudes(form):
    """rows scaled by powers of two down to 2^-118 (operand elements down to about 2^-120) and columns down to 2^-22
    (products down to 2^-140 and below).  Derived, not fitted: an element below 2^-117 may lose its lo piece (|lo| <= 2^-9 |x|
    falls below bf16's smallest normal 2^-126), which costs at most 2^-8 of each of its products; a product below 2^-126
    may flush.  So  |err| <= 3e-5 sum_big |a||b| + 2^-8 sum_small |a||b| + 2^-126 x (kept products),  big = both elements
    at or above 2^-117, kept products = 3 per term (hi hi, hi lo, lo hi).  The report line gives the worst ratio with and
    without the second term (a ratio <= 1 without it: the MFMA keeps bf16 denormals)."""
    from sigma_amd import gemm
    M, N, K = (8000, 132, 200) if form == "tn" else (300, 200, 132)
    rows, cols = (N, K) if form == "tn" else (M, N)
    r, c = _pow2_scales(rows, 131, lo=-118, hi=0), _pow2_scales(cols, 132, lo=-22, hi=0)
    if form == "nt":
        a, b = _rand(M, K, seed=133) * r[:, None], _rand(N, K, seed=134, scale=0.05) * c[:, None]
        got, a64, b64 = gemm.gemm_nt(a, b), a.double(), b.double().t()
    elif form == "nn":
        a, b = _rand(M, K, seed=133) * r[:, None], _rand(K, N, seed=134, scale=0.05) * c[None, :]
        got, a64, b64 = gemm.gemm_nn(a, b), a.double(), b.double()
    else:
        a, b = _rand(M, N, seed=133, scale=0.1) * r[None, :], _rand(M, K, seed=134) * c[None, :]
        got, a64, b64 = gemm.gemm_tn(a, b), a.double().t(), b.double()
    thr = 2.0 ** -117
    assert float(a64.abs()[a64 != 0].min()) < 2.0 ** -119 and bool(torch.isfinite(got).all())
    big = lambda t: torch.where(t.abs() >= thr, t.abs(), torch.zeros_like(t))
    total, s_big = _bound(a64, b64), big(a64) @ big(b64)
    assert float(r.min()) * float(c.min()) == 2.0 ** -140
    kept = 3 * a64.shape[1] * 2.0 ** -126
    err = (got.double() - a64 @ b64).abs()
    with_lo = float((err / (3e-5 * s_big + 2.0 ** -8 * (total - s_big) + kept)).max())
    without = float((err / (3e-5 * total + kept)).max())
    REPORT[form] = (with_lo, without)
    print(f"  small magnitudes {form}: worst err / bound = {with_lo:.3g}; without the lost-lo term {without:.3g}")
    assert with_lo <= 1.0, f"{form}: err / bound = {with_lo:.3g}"


def test_report_whether_a_lo_piece_below_the_bf16_normal_range_survives():
    """x = (1 + 2^-9) 2^-118 splits into hi = 2^-118 and lo = 2^-127, a bf16 denormal; against b = 2^10 both products are
    normal in fp32 (2^-108, 2^-117), so C = K x b exactly when the conversion and the MFMA keep bf16 denormals and
    K 2^-108 when they flush them.  Either is inside the contract (the second term of the small-magnitude bound); the line
    printed says which this device does."""
    from sigma_amd import gemm
    M, K, N = 32, 32, 32
    x = (1.0 + 2.0 ** -9) * 2.0 ** -118
    a, b = torch.full((M, K), x, device=DEV), torch.full((N, K), 2.0 ** 10, device=DEV)
    got = gemm.gemm_nt(a, b)
    kept, flushed = K * x * 2.0 ** 10, K * 2.0 ** -108
    assert bool(((got == kept) | (got == flushed)).all()), got.flatten()[:4]
    which = "kept" if bool((got == kept).all()) else ("flushed" if bool((got == flushed).all()) else "mixed")
    REPORT["lo denormal"] = which
    print(f"  a lo piece of 2^-127 (bf16 denormal) is {which}")
