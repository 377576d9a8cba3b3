"""Deterministic mode on the MI355X (sigma_amd/deterministic.py): every backward family through the C ABI with the
deterministic bit (all of dA / dD / ddelta_bias written, same values as the atomic path to summation order), bitwise
repeats at the real launch sizes of the step (GPU against GPU: no CPU oracle at full size), the depthwise conv and the
residual scale, and the whole training step (eager and graph-replayed) in a child process.  Values: the per-workgroup
slots of the workspace against the written dA / dD / ddelta_bias (fp64), and the fixture models against the reference's
own model under the flag (child process).  Every test that sets torch's flag restores it."""
import contextlib
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from sigma_amd import _capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


@contextlib.contextmanager
def deterministic(on=True):
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    fill = torch.utils.deterministic.fill_uninitialized_memory
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
        torch.utils.deterministic.fill_uninitialized_memory = fill


def _core():
    from sigma_amd import selective_scan_cuda_core as core
    return core


def _problem(batch, KD, L, N, G, ush, dtype=torch.float32, seed=0):
    """model-like operands on the GPU (magnitudes of a fresh SS2D block); u / dout hold the rows of every 2^ush-th group"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    A = -torch.arange(1, N + 1, dtype=torch.float32, device=DEV).repeat(KD, 1) * (1 + 0.05 * torch.rand(KD, N, generator=g, device=DEV))
    u = r(batch, KD >> ush, L).to(dtype)
    delta = (0.5 * r(batch, KD, L)).to(dtype)
    B, C = r(batch, G, N, L).to(dtype), r(batch, G, N, L).to(dtype)
    D = 1.0 + 0.1 * r(KD)
    bias = -3.0 + 0.5 * r(KD)
    dout = r(batch, KD >> ush, L).to(dtype)
    return u, delta, A, B, C, D, bias, dout


def _bwd_capi(args, dout, x, pitch, mask, ush, flags, fill, ws_fill=None):
    """sigma_selective_scan_bwd called directly: dA / dD / ddelta_bias pre-filled with `fill`, the workspace with `ws_fill`
    (None: left as allocated); returns the seven gradients, the plan report and the workspace (fp32 view)"""
    core = _core()
    lib = _capi.load()
    u, delta, A, B, C, D, bias = args
    batch, dim, L = delta.shape
    N, G = A.shape[1], B.shape[1]
    du, ddelta = torch.empty_like(delta), torch.empty_like(delta)
    dA = torch.full((dim, N), fill, device=DEV)
    dD, dbias = torch.full((dim,), fill, device=DEV), torch.full((dim,), fill, device=DEV)
    dB = torch.empty(B.shape, device=DEV)
    dC = torch.empty(C.shape, device=DEV)
    bp = _capi.BwdParams()
    core._fill_fwd(bp.fwd, u, delta, A, B, C, D, bias, None, x, True, (batch, dim, L, N, G), mask, ush, pitch, 0)
    bp.dout_group_shift, bp.flags = ush, flags
    bp.dout, bp.du, bp.ddelta = dout.data_ptr(), du.data_ptr(), ddelta.data_ptr()
    bp.dA, bp.dB, bp.dC, bp.dD, bp.ddelta_bias = dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), dD.data_ptr(), dbias.data_ptr()
    bp.dout_batch_stride, bp.dout_d_stride = dout.stride(0), dout.stride(1)
    bp.du_batch_stride, bp.du_d_stride = du.stride(0), du.stride(1)
    bp.ddelta_batch_stride, bp.ddelta_d_stride = ddelta.stride(0), ddelta.stride(1)
    bp.dA_d_stride, bp.dA_dstate_stride = dA.stride(0), dA.stride(1)
    bp.dB_batch_stride, bp.dB_group_stride, bp.dB_dstate_stride = dB.stride()[:3]
    bp.dC_batch_stride, bp.dC_group_stride, bp.dC_dstate_stride = dC.stride()[:3]
    plan = (ctypes.c_int32 * 6)()
    assert lib.sigma_scan_bwd_plan(ctypes.byref(bp), ctypes.byref(plan)) == 0, _capi.last_error()
    ws_bytes = lib.sigma_scan_bwd_workspace_bytes(ctypes.byref(bp))
    assert ws_bytes >= 0, _capi.last_error()
    ws = torch.empty(max(ws_bytes, 16) // 4, dtype=torch.float32, device=DEV)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    bp.workspace, bp.workspace_bytes = ws.data_ptr(), ws_bytes
    _capi.check(lib.sigma_selective_scan_bwd(ctypes.byref(bp), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "bwd")
    torch.cuda.synchronize()
    return [du, ddelta, dA, dB, dC, dD, dbias], list(plan), ws[:ws_bytes // 4]


# (batch, KD, L, N, G, rev_mask, u_gshift, pitch, dtype, family) -- small launches that force each backward family
FAMILIES = [
    (2, 256, 600, 16, 4, 0b1010, 1, 16, torch.float32, "Bwdr"),
    (1, 256, 4800, 16, 4, 0b1010, 1, 16, torch.float32, "Bwdr"),       # sequence segments
    (2, 256, 1600, 16, 4, 0b1010, 1, 160, torch.float32, "Bwd4"),
    (1, 256, 9600, 16, 4, 0b1010, 1, 160, torch.float32, "Bwd4"),      # sequence segments
    (2, 256, 1600, 4, 4, 0b1010, 1, 640, torch.float32, "Bwd2"),
    (2, 256, 1600, 16, 4, 0b1010, 1, 320, torch.float32, "Bwd2"),
    (2, 256, 1280, 16, 4, 0b1010, 1, 640, torch.bfloat16, "Bwd2"),     # 16-bit IO
    (8, 3072, 320, 4, 4, 0b1010, 1, 320, torch.float32, "Bwd3"),
    (2, 128, 3000, 16, 2, 0, 0, 0, torch.float32, "Bwd"),
]


@pytest.mark.parametrize("shape", FAMILIES, ids=[f"{s[9]}-{s[0]}x{s[1]}x{s[2]}xN{s[3]}-{str(s[8])[6:]}" for s in FAMILIES])
def test_every_family_writes_all_row_gradients(shape):
    from tests.test_deterministic_cpu import family_of
    batch, KD, L, N, G, mask, ush, pitch, dtype, family = shape
    u, delta, A, B, C, D, bias, dout = _problem(batch, KD, L, N, G, ush, dtype, seed=3)
    core = _core()
    args = (u, delta, A, B, C, D, bias)
    from tests.test_stream_fp64_gpu import IO_DTYPES, recording, scan_case_keys
    with recording() as launched:
        _, x = core.fwd_ext(*args, True, rev_mask=mask, u_gshift=ush, ckpt_pitch=pitch)
        ref, plan, _ = _bwd_capi(args, dout, x, pitch, mask, ush, 0, 0.0)           # the accumulating contract, zeroed
        det, plan_d, _ = _bwd_capi(args, dout, x, pitch, mask, ush, _capi.SIGMA_SCAN_BWD_DETERMINISTIC, float("nan"), float("nan"))
    assert launched == scan_case_keys(*shape[:8], IO_DTYPES[dtype], det=(False, True))    # the census keys of this case
    assert plan == plan_d and family_of(plan) == family
    names = ["du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias"]
    for name, a, b in zip(names, det, ref):
        a, b = a.float(), b.float()
        assert torch.isfinite(a).all(), f"{name}: not every element written"
        err = (a - b).abs().max().item()
        assert err <= 1e-5 * b.abs().max().item(), f"{name}: {err:.3e} vs max {b.abs().max().item():.3e}"
    # the flag-clear contract is kept: dA / dD / ddelta_bias are ADDED to what the caller passes
    acc, _, _ = _bwd_capi(args, dout, x, pitch, mask, ush, 0, 1.0)
    for name, a, b in zip(names[5:] + names[2:3], acc[5:] + acc[2:3], ref[5:] + ref[2:3]):
        torch.testing.assert_close(a, b + 1.0, rtol=1e-5, atol=1e-5 * (1 + b.abs().max().item()), msg=name)


# real launches of the sigma_small 480 x 640 step (tests/test_scan_gpu.py FULL_LAUNCHES), through the binding with
# torch's flag: three backwards must be byte-identical in all seven gradients
REPEAT = [
    (16, 3072, 1200, 16, 4, 0b1010, 1, 16),      # row-lane
    (16, 768, 19200, 16, 4, 0b1010, 1, 160),     # quad-row
    (8, 768, 19200, 4, 4, 0b1010, 1, 640),       # 64-lane
    (1, 768, 19200, 16, 4, 0b1010, 1, 16),       # row-lane with sequence segments
]


@pytest.mark.parametrize("shape", REPEAT, ids=["x".join(map(str, s[:3])) + f"xN{s[3]}-p{s[7]}" for s in REPEAT])
def test_bitwise_repeat_at_real_sizes(shape):
    batch, KD, L, N, G, mask, ush, pitch = shape
    core = _core()
    u, delta, A, B, C, D, bias, dout = _problem(batch, KD, L, N, G, ush, seed=7)
    args = (u, delta, A, B, C, D, bias)
    with deterministic():
        _, x = core.fwd_ext(*args, True, rev_mask=mask, u_gshift=ush, ckpt_pitch=pitch)
        first = core.bwd_ext(*args, dout, x, True, rev_mask=mask, u_gshift=ush, dout_gshift=ush, ckpt_pitch=pitch)
        for _ in range(2):
            again = core.bwd_ext(*args, dout, x, True, rev_mask=mask, u_gshift=ush, dout_gshift=ush, ckpt_pitch=pitch)
            for i, (a, b) in enumerate(zip(first, again)):
                assert torch.equal(a, b), f"gradient {i} differs between two deterministic backwards"
            del again


SLOTS = REPEAT + [(1, 768, 19200, 16, 4, 0b1010, 1, 160)]       # + quad-row with sequence segments


@pytest.mark.parametrize("shape", SLOTS, ids=["x".join(map(str, s[:3])) + f"xN{s[3]}-p{s[7]}" for s in SLOTS])
def test_slots_add_up_to_the_written_row_gradients(shape):
    """The per-workgroup slots of a deterministic backward through the C ABI, workspace NaN-filled: the slot region is the
    tail of the workspace, [rpart_K][dim][N + 2] floats (columns dA[0..N), dD, ddelta_bias; rpart_K = batch x segments),
    exactly what the flag adds to the workspace query; every slot is written (finite), and the written dA / dD /
    ddelta_bias equal the fp64 sum of their rpart_K slots within (rpart_K + 1) u sum_k |slot[k]|
    (reduce_partials_det_kernel: rpart_K serial fp32 adds).  Negative control: the sum without the last slot."""
    from tests.test_deterministic_cpu import bwd_params, segments_of
    from tests.test_stream_fp64_gpu import check, rejects
    batch, KD, L, N, G, mask, ush, pitch = shape
    lib = _capi.load()
    flag = _capi.SIGMA_SCAN_BWD_DETERMINISTIC
    u, delta, A, B, C, D, bias, dout = _problem(batch, KD, L, N, G, ush, seed=5)
    args = (u, delta, A, B, C, D, bias)
    _, x = _core().fwd_ext(*args, True, rev_mask=mask, u_gshift=ush, ckpt_pitch=pitch)
    det, plan, ws = _bwd_capi(args, dout, x, pitch, mask, ush, flag, float("nan"), float("nan"))
    K = batch * segments_of(plan)
    assert K > 1, "one slot per row: nothing to check"
    with_flag = lib.sigma_scan_bwd_workspace_bytes(ctypes.byref(bwd_params(batch, KD, L, N, G, mask, ush, pitch, 0, flag)))
    without = lib.sigma_scan_bwd_workspace_bytes(ctypes.byref(bwd_params(batch, KD, L, N, G, mask, ush, pitch, 0)))
    assert with_flag - without == K * KD * (N + 2) * 4, "the slot region is not [batch x segments][dim][N + 2] floats"
    assert ws.numel() * 4 == with_flag
    slots = ws[ws.numel() - K * KD * (N + 2):].view(K, KD, N + 2)
    assert torch.isfinite(slots).all(), f"{int((~torch.isfinite(slots)).sum())} slot entries not written"
    s64 = slots.double()
    ref, S = s64.sum(0), s64.abs().sum(0)
    got = torch.cat([det[2], det[5][:, None], det[6][:, None]], 1)
    check("det slots", got, ref, S, K + 1, "dA | dD | ddelta_bias against the sum of the slots")
    rejects(got, s64[:-1].sum(0), S, K + 1, "the sum without the last slot")


def _dw_capi(x, w, b, g2, flags, fill):
    lib = _capi.load()
    B, d, H, W = x.shape
    dw = torch.full_like(w, fill)
    db = torch.full((d,), fill, device=DEV)
    dx = torch.empty_like(x)
    gpre = torch.empty_like(x)
    p = _capi.DwConvParams()
    p.batch, p.channels, p.height, p.width, p.n_orders, p.flags = B, d, H, W, 2, flags
    p.x, p.weight, p.bias, p.g2, p.gpre = x.data_ptr(), w.data_ptr(), b.data_ptr(), g2.data_ptr(), gpre.data_ptr()
    p.dweight, p.dbias, p.dx = dw.data_ptr(), db.data_ptr(), dx.data_ptr()
    n = lib.sigma_dwconv3x3_silu_bwd_workspace_bytes(ctypes.byref(p))
    assert n >= 0
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=DEV)
    p.workspace, p.workspace_bytes = ws.data_ptr(), n
    assert lib.sigma_dwconv3x3_silu_bwd(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return dx, dw, db


@pytest.mark.parametrize("shape", [(16, 192, 120, 160), (2, 64, 15, 20)], ids=["stage0-tiled", "plane-in-lds"])
def test_dwconv_backward_written_and_repeatable(shape):
    B, d, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(B, d, H, W, generator=g, device=DEV)
    w = 0.3 * torch.randn(d, 1, 3, 3, generator=g, device=DEV)
    b = 0.1 * torch.randn(d, generator=g, device=DEV)
    g2 = torch.randn(B, 2, d, H * W, generator=g, device=DEV)
    ref = _dw_capi(x, w, b, g2, 0, 0.0)
    det = _dw_capi(x, w, b, g2, _capi.SIGMA_DWCONV_DETERMINISTIC, float("nan"))
    for name, a, r in zip(("dx", "dweight", "dbias"), det, ref):
        assert torch.isfinite(a).all(), name
        assert (a - r).abs().max().item() <= 1e-5 * r.abs().max().item(), name
    # the binding under torch's flag: bitwise repeat
    from sigma_amd.ss2d_fused import dwconv_silu_two_orders
    outs = []
    with deterministic():
        for _ in range(3):
            xs, ws_, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
            dwconv_silu_two_orders(xs, ws_, bs).backward(g2)
            outs.append((xs.grad, ws_.grad, bs.grad))
    for o in outs[1:]:
        assert all(torch.equal(a, c) for a, c in zip(outs[0], o))


def test_colscale_backward_written_and_repeatable():
    lib = _capi.load()
    rows, C = 16 * 120 * 160, 96
    g = torch.Generator(device=DEV).manual_seed(12)
    dy, x = torch.randn(rows, C, generator=g, device=DEV), torch.randn(rows, C, generator=g, device=DEV)
    s = torch.randn(C, generator=g, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dx0, ds0 = torch.empty_like(x), torch.zeros(C, device=DEV)
    assert lib.sigma_colscale_bwd(dy.data_ptr(), x.data_ptr(), s.data_ptr(), dx0.data_ptr(), ds0.data_ptr(), rows, C, st) == 0
    n = lib.sigma_colscale_bwd_workspace_bytes(rows, C)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    res = []
    for _ in range(3):
        dx, ds = torch.empty_like(x), torch.full((C,), float("nan"), device=DEV)
        assert lib.sigma_colscale_bwd_ws(dy.data_ptr(), x.data_ptr(), s.data_ptr(), dx.data_ptr(), ds.data_ptr(), rows, C,
                                         ws.data_ptr(), n, st) == 0
        res.append((dx, ds))
    torch.cuda.synchronize()
    assert torch.isfinite(res[0][1]).all() and torch.equal(res[0][0], dx0)
    assert (res[0][1] - ds0).abs().max().item() <= 1e-5 * ds0.abs().max().item()
    assert all(torch.equal(r[1], res[0][1]) for r in res[1:])


def test_whole_training_step_is_bitwise_reproducible():
    """Two training steps (forward, backward, AdamW) of a fixture-size model with DropPath active, from identical state
    under torch's flag: eager twice and graph-replayed twice, every parameter and gradient bitwise equal between the two
    runs of each kind.  In a child process: the flag and CUBLAS_WORKSPACE_CONFIG stay out of this one."""
    env = dict(os.environ, CUBLAS_WORKSPACE_CONFIG=":4096:8")
    r = subprocess.run([sys.executable, "-m", "tests.deterministic_step_worker"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, f"worker exit {r.returncode}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    assert "[deterministic_step_worker] done" in r.stdout


def test_fixture_models_match_the_reference_under_the_flag():
    """The model-level VALUES of deterministic mode: tests/deterministic_model_worker.py runs the fixture comparison of
    tests/test_model_gpu.py (both fixtures, split3 GEMMs, automatic pitch, the same tolerances) under torch's flag, in a
    child process."""
    env = dict(os.environ, CUBLAS_WORKSPACE_CONFIG=":4096:8", SIGMA_GEMM="split3")
    env.pop("SIGMA_CKPT_PITCH", None)                                # automatic pitch
    r = subprocess.run([sys.executable, "-m", "tests.deterministic_model_worker"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, f"worker exit {r.returncode}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    assert "[deterministic_model_worker] done" in r.stdout
