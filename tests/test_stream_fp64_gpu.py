"""fp64 parity of the stream kernels (LayerNorm, depthwise conv + SiLU, cross merge / split, transpose2d, pair_sum_add,
bilinear x2, the ChannelAttention plane ops, colscale_bwd, softmax cross entropy) at the paths the host code selects;
run with -m gpu.

Census.  ``_capi.load`` is wrapped by a recorder that keys every stream-kernel and GEMM call by the path its host code
picks (``launch_key``, a mirror of the selection rules with their source lines).  One forward + backward of sigma_small
(480x640) and sigma_base (720x1280) must meet only keys of ``COVERED``: a model or dispatch change that opens an untested
path fails ``test_census_of_both_models_is_covered``.  The stream-kernel cases below record their own launches and assert
that they reach the key ``COVERED`` assigns to them.

References are written from the formula in fp64 on the device (no fp32 op, no CPU oracle); gradients come from fp64
autograd of the same reference.

Tolerances.  u = 2^-24.  An fp32 sum of n terms computed in an order of serial depth d (longest chain of dependent
adds) differs from the exact sum by at most ~d u sum|terms|; a product adds one u of its magnitude.  For every output
the test computes, in fp64, S = the sum of |terms| that forms it (including the propagated error of its inputs, e.g. the
row statistics of a LayerNorm), and asserts  |got - ref| <= K u S  with K = (serial depth of the kernel's summation
order) + (a few roundings of the elementwise tail: rsqrt, exp2, rcp are within 2 ulp on gfx950), written out per
family.  Each family also has a NEGATIVE CONTROL: a plausible wrong fp64 variant (eps outside the sqrt, replicate
padding, swapped scan orders, align_corners=True, a missing last row block, ...) that the kernel's output must FAIL
under the same bound, i.e. the bound is tight enough to see that error.  Only reference code runs in the controls.

Guard bands.  Every kernel output is written into the interior of a larger buffer prefilled with NaN; the margins
(>= one row + 64 floats, in the same allocation) must still be all NaN afterwards, so an overrun that lands in owned
memory is detected without a fault.
"""
from __future__ import annotations

import contextlib
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
WORST: dict = {}             # family -> worst error / bound ratio seen (printed by the last test)


# ---------------------------------------------------------------------------------------------------------------------
# path keys: a mirror of the host-side selection

def ln_nv(C: int) -> int:
    """csrc/layernorm.hip dispatch_nv (:296): NV = ceil(C / 256) rounded up to {1, 2, 3, 4, 6, 8}"""
    nv = (C + 255) // 256
    return {5: 6, 7: 8}.get(nv, nv)


def dw_plane(H: int, W: int) -> bool:
    """csrc/dwconv.hip plane_lds_bytes (:347): two (H + 2) x ((W + 2) | 1) fp32 images in <= 48 KiB -> whole-plane kernel"""
    return 2 * (H + 2) * ((W + 2) | 1) * 4 <= 48 * 1024


def _al16(v) -> bool:
    return int(v or 0) % 16 == 0


def _ptr(a):
    return a.value if isinstance(a, ctypes.c_void_p) else a


def launch_key(lib, name, args):
    """the path a stream-kernel / GEMM call takes, from its arguments (None: not a recorded symbol)"""
    a = [_ptr(x) for x in args]
    if name in ("sigma_layernorm_fwd", "sigma_layernorm_bwd"):
        p = args[0]._obj
        k = ("ln_fwd" if name.endswith("fwd") else "ln_bwd", ln_nv(p.channels), bool(p.gate), bool(p.row_scale))
        return k + ((bool(p.dx_add),) if name.endswith("bwd") else ())
    if name.startswith("sigma_dwconv3x3_silu"):
        p = args[0]._obj
        L = p.height * p.width
        strided = (p.x_batch_stride, p.x_channel_stride) not in ((0, 0), (p.channels * L, L))     # dwconv.hip plane_strides
        k = ("dw_" + name[-3:], "plane" if dw_plane(p.height, p.width) else "tiled", p.n_orders, strided)
        return k + ((bool(p.flags & 1),) if name.endswith("bwd") else ())                         # SIGMA_DWCONV_DETERMINISTIC
    if name in ("sigma_softmax_ce_fwd", "sigma_softmax_ce_bwd"):
        nc = int(a[3] if name.endswith("fwd") else a[5])
        return ("ce_" + name[-3:], "reg" if nc // 4 <= 16 else "generic")                        # pointwise.hip:274 dispatch_nc4
    if name == "sigma_plane_pool":                                                                # pointwise.hip:338
        return ("plane_pool", "vec" if a[2] % 4 == 0 and _al16(a[0]) else "scalar")
    if name == "sigma_plane_dot":                                                                 # pointwise.hip:348
        return ("plane_dot", "vec" if a[4] % 4 == 0 and _al16(a[0]) and _al16(a[1]) else "scalar")
    if name == "sigma_plane_scale":                                                               # pointwise.hip:357
        return ("plane_scale", "vec" if a[4] % 4 == 0 and _al16(a[0]) and _al16(a[2]) else "scalar")
    if name == "sigma_plane_gate_bwd":                                                            # pointwise.hip:383
        p = args[0]._obj
        return ("plane_gate_bwd", "vec" if p.hw % 4 == 0 and _al16(p.g) and _al16(p.x) and _al16(p.dx) else "scalar")
    if name == "sigma_pair_sum_add":                                                              # merge.hip:250
        return ("pair_sum_add", "vec" if a[3] % 4 == 0 and _al16(a[0]) and _al16(a[1]) else "scalar")
    if name == "sigma_colscale_bwd":                                                              # pointwise.hip:370
        return ("colscale_bwd", 256 // (int(a[6]) // 4))
    if name == "sigma_colscale_bwd_ws":                                                           # pointwise.hip:423
        return ("colscale_bwd_ws", 256 // (int(a[6]) // 4))
    if name in SCAN_SYMBOLS:
        return scan_key(lib, name, args[0]._obj)
    if name == "sigma_cross_merge_nhwc":
        return ("merge",)
    if name == "sigma_cross_split_nhwc":
        return ("split",)
    if name == "sigma_transpose2d":
        return ("transpose",)
    if name == "sigma_upsample2x_nhwc":
        return ("upsample", "adjoint" if a[6] else "fwd")
    if name in ("sigma_gemm_nt_split3", "sigma_gemm_nn_split3", "sigma_gemm_tn_split3"):
        p = args[0]._obj
        form = name[11:13]
        from sigma_amd import _capi
        need = int(lib.sigma_gemm_workspace_bytes(ctypes.byref(p), _capi.GEMM_FORMS[form]))   # gemm_split.hip plan_gemm
        stage = "own" if need == 0 else ("two-stage" if p.workspace and p.workspace_bytes >= need else "atomic")
        plan = _capi.gemm_plan(p, form, lib) or {}                  # sigma_gemm_plan: which kernel runs, with which epilogue
        return ("gemm", form, p.pieces or 2, p.batch > 1, p.a_mod > 0, bool(p.c_mod > 0 and p.batch > p.c_mod),
                bool(p.k_slices), p.t_cols > 0, int(bool(p.residual)) + int(bool(p.residual2)), bool(p.bias),
                bool(p.accumulate), plan.get("bn", 0), plan.get("epilogue", "refused"), stage)
    return None


SCAN_SYMBOLS = ("sigma_selective_scan_fwd", "sigma_selective_scan_bwd")


def scan_key(lib, name, p):
    """the kernel family a scan launch takes (the planner's report, decoded as tests/test_deterministic_cpu.py does), the
    deterministic bit (backward), the IO dtype (0 f32, 1 f16, 2 bf16) and whether the sequence is cut into segments"""
    from tests.test_deterministic_cpu import family_of, fwd_family_of, segments_of
    plan = (ctypes.c_int32 * 6)()
    if name.endswith("fwd"):
        if lib.sigma_scan_fwd_plan(ctypes.byref(p), ctypes.byref(plan)) != 0:
            return ("scan_fwd", "refused")
        fam = fwd_family_of(list(plan))
        return ("scan_fwd", fam, int(p.io_dtype), fam == "Fwdr" and plan[4] > 1)
    if lib.sigma_scan_bwd_plan(ctypes.byref(p), ctypes.byref(plan)) != 0:
        return ("scan_bwd", "refused")
    return ("scan_bwd", family_of(list(plan)), bool(p.flags & 1), int(p.fwd.io_dtype), segments_of(list(plan)) > 1)


def scan_case_keys(batch, KD, L, N, G, mask, ush, pitch, io=0, det=(False,)):
    """the scan keys of a test case's forward and backward(s), planned for its (contiguous) operands -- no GPU needed"""
    from tests.test_deterministic_cpu import bwd_params
    from sigma_amd import _capi
    lib = _capi.load()
    bp = bwd_params(batch, KD, L, N, G, mask, ush, pitch, io)
    keys = [scan_key(lib, "sigma_selective_scan_fwd", bp.fwd)]
    for d in det:
        keys.append(scan_key(lib, "sigma_selective_scan_bwd",
                             bwd_params(batch, KD, L, N, G, mask, ush, pitch, io, _capi.SIGMA_SCAN_BWD_DETERMINISTIC if d else 0)))
    return keys


class _Recorder:
    """stands in for the ctypes library: records (symbol, key) of every keyed call, then forwards it"""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not (name.startswith("sigma_") and (name in _OPS or name in SCAN_SYMBOLS or
                                               name.startswith("sigma_gemm_") and name.endswith("split3"))):
            return fn

        def call(*args):
            self._log.append(launch_key(self._lib, name, args))
            return fn(*args)
        return call


def _ops():
    from sigma_amd import _capi
    return set(_capi.OPS_SYMBOLS) - {"sigma_layernorm_bwd_partial_rows"}


_OPS = set()


@contextlib.contextmanager
def recording():
    """sigma_amd._capi.load replaced by a recorder for the block; yields the list the keys are appended to"""
    from sigma_amd import _capi
    global _OPS
    _OPS = _ops()
    real = _capi.load
    log: list = []
    rec = _Recorder(real(), log)
    _capi.load = lambda: rec
    try:
        yield log
    finally:
        _capi.load = real


@pytest.fixture
def record():
    """the recorder of ``recording`` around one test"""
    with recording() as log:
        yield log


# Every path the two models take -> the real shape it is tested at (cases below; GEMM keys: tests/test_gemm_gpu.py)
COVERED = {}


def covers(key, where):
    COVERED.setdefault(key, where)
    return key


# ---------------------------------------------------------------------------------------------------------------------
# helpers

def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(shape, row: int, offset: int = 0):
    """(buffer, view) of `shape` inside a NaN-filled buffer; margins of row + 64 floats (rounded to 4) on both sides;
    ``offset`` (floats) shifts the view off its 16-byte alignment"""
    n = math.prod(shape)
    m = (row + 64 + 3) // 4 * 4
    buf = torch.full((n + 2 * m + offset,), float("nan"), device=DEV)
    return buf, buf[m + offset:m + offset + n].view(*shape), (m + offset, n)


def _intact(g, what):
    buf, _, (start, n) = g
    assert bool(torch.isnan(buf[:start]).all()) and bool(torch.isnan(buf[start + n:]).all()), f"{what}: guard band written"


def _ratio(got, ref, S, K):
    err = (got.double() - ref).abs()
    return float((err / (K * U * S + 1e-300)).max())


def check(family, got, ref, S, K, what):
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    r = _ratio(got, ref, S, K)
    WORST[family] = max(WORST.get(family, 0.0), r)
    assert r <= 1.0, f"{what}: max |err| / (K u S) = {r:.3g} (K = {K})"
    return r


def rejects(got, wrong, S, K, what):
    """negative control: the kernel's output must FAIL the bound against a plausible wrong reference"""
    r = _ratio(got, wrong, S, K)
    assert r > 1.0, f"{what}: the bound cannot tell the kernel from the wrong variant (ratio {r:.3g})"


def _rand(*shape, seed=0, scale=1.0, mean=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale + mean


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm

def _ln_ref(x, gamma, beta, eps, z=None, rs=None, rows_per=1, unbiased=False, eps_out=False):
    mu = x.mean(-1, keepdim=True)
    var = x.var(-1, keepdim=True, unbiased=unbiased)
    r = 1.0 / (var.sqrt() + eps) if eps_out else torch.rsqrt(var + eps)
    xh = (x - mu) * r
    y = xh * gamma + beta
    s = None
    if z is not None:
        s = z * torch.sigmoid(z)
        y = y * s
    if rs is not None:
        y = y * rs.repeat_interleave(rows_per)[:, None]
    return y, xh, r, mu


# (rows, C, variant, where): variant = plain / dx_add / gated / gated_rs
LN_CASES = [
    # sigma_small at batch 8 (Siamese encoder batch 16), sigma_base at batch 1
    (16 * 19200, 96, "dx_add", "s enc stage1 norm 16x120x160x96"),
    (16 * 19200, 192, "gated_rs", "s enc stage1 out_norm d_inner 192"),
    (16 * 4800, 384, "gated_rs", "s enc stage2 out_norm 384"),
    (16 * 1200, 768, "gated_rs", "s enc stage3 out_norm 768"),
    (16 * 300, 1536, "gated_rs", "s enc stage4 out_norm 1536"),
    (16 * 1200, 768, "plain", "s PatchMerging norm 4x192"),
    (8 * 19200, 96, "plain", "s decoder norm 8x120x160x96"),
    (8 * 19200, 192, "gated", "s gated norm, C = 192 without a row factor"),
    (16 * 1200, 384, "dx_add", "s enc stage3 norm 16x30x40x384"),
    (16 * 1200, 384, "plain", "s PatchMerging norm 4x96 / decoder 384"),
    (3600, 1024, "dx_add", "b stage-3 sized rows, C = 1024 (NV=4)"),
    (3600, 1024, "plain", "b PatchMerging norm 4x256 (NV=4)"),
    (3600, 1024, "gated_rs", "b out_norm d_inner 1024 (NV=4)"),
    (920, 2048, "gated_rs", "b out_norm d_inner 2048 (NV=8)"),
    (920, 2048, "gated", "b gated 2048 (NV=8)"),
    # selector boundaries: NV buckets and their rounding-up cases (5 -> 6, 7 -> 8)
    (2000, 256, "plain", "NV=1 edge"), (2000, 260, "gated", "NV=2 first"), (2000, 768, "dx_add", "NV=3 edge"),
    (2000, 772, "gated_rs", "NV=4 first"), (2000, 1028, "plain", "NV=5 -> 6"), (2000, 1028, "gated", "NV=5 -> 6 gated"),
    (2000, 1280, "dx_add", "NV=5 -> 6 edge"), (2000, 1536, "gated_rs", "NV=6 edge"), (2000, 1540, "plain", "NV=7 -> 8"),
    (2000, 1540, "gated_rs", "NV=7 -> 8 gated"), (2000, 1792, "dx_add", "NV=7 -> 8 edge"), (2000, 1796, "gated", "NV=8 first"),
    (2000, 2048, "plain", "NV=8 edge"), (2001, 2048, "dx_add", "NV=8 odd rows"), (3, 1024, "gated_rs", "NV=4 three rows"),
]


def _ln_keys(C, variant):
    gate, rs, dxa = variant.startswith("gated"), variant == "gated_rs", variant == "dx_add"
    return ("ln_fwd", ln_nv(C), gate, rs), ("ln_bwd", ln_nv(C), gate, rs, dxa)


for _rows, _C, _v, _w in LN_CASES:
    for _k in _ln_keys(_C, _v):
        covers(_k, f"test_layernorm_against_fp64[{_rows}x{_C}-{_v}] ({_w})")


@pytest.mark.parametrize("case", LN_CASES, ids=[f"{r}x{c}-{v}" for r, c, v, _ in LN_CASES])
def test_layernorm_against_fp64(case, record):
    """y = (x - mean) rsqrt(var_biased + eps) gamma + beta  [* silu(z)] [* row_scale[sample]], backward dx [+ dx_add],
    dgamma, dbeta [, dz].

    Kernel order (csrc/layernorm.hip): a lane sums its 4 NV columns serially, then six DPP levels: row sums of serial
    depth d = 4 NV + 6.  mean: d u sum|x| / C; the centred sum of squares: d u sum (x-mu)^2 + the mean's error; rsqrt
    2 ulp.  So  y: K = d + 12,  S = (|gamma| (|xh| + r mean|x|) + |beta|) |silu z| |rs|  (silu: exp2 + rcp, 4 ulp).
    dx = r (g - mean g - xh mean(g xh)), g = dy gamma silu(z) rs: row sums of depth d plus the error of r and xh:
    K = 2 d + 16,  S = r (|g| + mean|g| + |xh| mean|g xh|) + |dx_add|.
    dgamma / dbeta are column sums over the rows: each wave walks rows wave, wave + nw, ... (serial, ceil(rows / 4 G)
    deep, G = workgroups), the 4 waves of a workgroup meet in LDS (4), ln_reduce_kernel adds the G partial rows (16
    threads x ceil(G / 16) serial, then 16): K = ceil(rows / 4G) + ceil(G / 16) + 20 + (d + 12 for dgamma's xh),
    S = sum |g_pre xh| resp. sum |g_pre| (g_pre = dy silu(z) rs).
    Negative controls: eps outside the sqrt (1 / (sqrt(var) + eps)), unbiased variance, dgamma without the last
    partial row block."""
    from sigma_amd import _capi
    rows, C, variant, _ = case
    gated, scaled, dxa = variant.startswith("gated"), variant == "gated_rs", variant == "dx_add"
    lib = _capi.load()
    eps = 1e-5
    nsamp = 2 if scaled and rows % 2 == 0 else 1
    # activations with a small variance (var ~ 4e-4), where eps matters: 2.5 % of var
    x = _rand(rows, C, seed=1, scale=0.02, mean=0.3)
    xc0 = x - x.mean(1, keepdim=True)
    gamma, beta = _rand(C, seed=2, scale=0.5, mean=1.0), _rand(C, seed=3, scale=0.1)
    zz = _rand(rows, 2 * C, seed=4) if gated else None            # the gate is the strided second half of (rows, 2C)
    z = zz[:, C:] if gated else None
    rsc = torch.tensor([1.0 / 0.9, 0.0][:nsamp] if nsamp == 2 else [1.0 / 0.9], device=DEV) if scaled else None
    dy = 25.0 * xc0 + _rand(rows, C, seed=5)          # correlated with xh: dgamma's row sums do not cancel
    dadd = _rand(rows, C, seed=6) if dxa else None

    gy, gmean, grstd = _guarded((rows, C), C), _guarded((rows,), 1), _guarded((rows,), 1)
    p = _capi.LayerNormParams()
    p.rows, p.channels, p.eps = rows, C, eps
    p.x, p.gamma, p.beta, p.y = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), gy[1].data_ptr()
    p.mean, p.rstd = gmean[1].data_ptr(), grstd[1].data_ptr()
    if gated:
        p.gate, p.gate_row_stride = z.data_ptr(), 2 * C
    if scaled:
        p.row_scale, p.rows_per_scale = rsc.data_ptr(), rows // nsamp
    _capi.check(lib.sigma_layernorm_fwd(ctypes.byref(p), _stream()), "layernorm_fwd")
    nw = int(lib.sigma_layernorm_bwd_partial_rows(rows, C))
    ws = torch.full((max(nw, 1) * 2 * C,), float("nan"), device=DEV)
    gdx, gdg, gdb = _guarded((rows, C), C), _guarded((C,), C), _guarded((C,), C)
    gdz = _guarded((rows, 2 * C), 2 * C) if gated else None
    p.dy, p.dx, p.dgamma, p.dbeta, p.workspace = dy.data_ptr(), gdx[1].data_ptr(), gdg[1].data_ptr(), gdb[1].data_ptr(), ws.data_ptr()
    if dxa:
        p.dx_add = dadd.data_ptr()
    if gated:
        p.dgate, p.dgate_row_stride = gdz[1][:, C:].data_ptr(), 2 * C
    _capi.check(lib.sigma_layernorm_bwd(ctypes.byref(p), _stream()), "layernorm_bwd")
    torch.cuda.synchronize()
    assert set(record) == set(_ln_keys(C, variant)), record
    for g, what in ((gy, "y"), (gmean, "mean"), (grstd, "rstd"), (gdx, "dx"), (gdg, "dgamma"), (gdb, "dbeta")):
        _intact(g, what)
    if gated:
        _intact(gdz, "dz")
        assert bool(torch.isnan(gdz[1][:, :C]).all()), "dz: the x half of the (rows, 2C) gradient buffer was written"

    x64, g64, b64 = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    z64 = z.double().requires_grad_() if gated else None
    rs64 = rsc.double() if scaled else None
    y64, xh, r, mu = _ln_ref(x64, g64, b64, eps, z64, rs64, rows // nsamp)
    y64.backward(dy.double())
    d = 4 * ln_nv(C) + 6
    with torch.no_grad():
        xd = x.double()
        s = (z64 * torch.sigmoid(z64)).abs() if gated else 1.0
        rsr = rs64.repeat_interleave(rows // nsamp)[:, None] if scaled else 1.0
        xha = xh.abs() + r * xd.abs().mean(-1, keepdim=True)      # |xh| + the error of the row mean, scaled by r
        S_ln = g64.abs() * xha + b64.abs()
        S_y = S_ln * s * rsr
        check("layernorm", gy[1], y64.detach(), S_y, d + 12, "y")
        check("layernorm", gmean[1], mu[:, 0], xd.abs().mean(-1), d + 2, "mean")
        check("layernorm", grstd[1], r[:, 0], r[:, 0], d + 12, "rstd")
        gpre = dy.double() * (s if gated else 1.0) * rsr
        gg = (gpre * g64).abs()
        S_dx = r * (gg + gg.mean(-1, keepdim=True) + xha * (gg * xha).mean(-1, keepdim=True))
        dx_ref = x64.grad + (dadd.double() if dxa else 0.0)
        if dxa:
            S_dx = S_dx + dadd.double().abs()
        check("layernorm", gdx[1], dx_ref, S_dx, 2 * d + 16, "dx")
        G = max(nw, 1)
        Kc = -(-rows // (4 * G)) + -(-G // 16) + 20
        S_dg = (gpre.abs() * xha).sum(0)
        check("layernorm", gdg[1], g64.grad, S_dg, Kc + d + 12, "dgamma")
        check("layernorm", gdb[1], b64.grad, gpre.abs().sum(0), Kc, "dbeta")
        if gated:
            sg = torch.sigmoid(z64)
            S_dz = (dy.double() * rsr).abs() * sg * (1 + z64.abs() * (1 - sg)) * S_ln
            check("layernorm", gdz[1][:, C:], z64.grad, S_dz, d + 20, "dz")
        # negative controls
        rejects(gy[1], _ln_ref(xd, gamma.double(), beta.double(), eps, z.double() if gated else None, rs64, rows // nsamp,
                               eps_out=True)[0], S_y, d + 12, "eps outside the sqrt")
        if C >= 256:
            rejects(gy[1], _ln_ref(xd, gamma.double(), beta.double(), eps, z.double() if gated else None, rs64, rows // nsamp,
                                   unbiased=True)[0], S_y, d + 12, "unbiased variance")
        if rows >= 4 * G:
            tail = rows % (4 * G) or 4 * G                         # the rows of the last walk step of the waves
            wrong = (gpre[:rows - tail] * xh[:rows - tail]).sum(0)
            if not (scaled and nsamp == 2):                        # (the second sample's factor is 0: its rows add nothing)
                rejects(gdg[1], wrong, S_dg, Kc + d + 12, "dgamma missing the last row block")


# ---------------------------------------------------------------------------------------------------------------------
# depthwise conv 3x3 + SiLU, two memory orders

def _dw_ref(x, w, b, pad="zeros"):
    """nine shifted adds: pre[h][w] = sum_{dy,dx} w[dy][dx] x[h + dy - 1][w + dx - 1] + b (zero or replicate padding)"""
    B, d, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1)) if pad == "zeros" else F.pad(x, (1, 1, 1, 1), mode="replicate")
    pre = b.view(1, d, 1, 1).expand(B, d, H, W).clone() if b is not None else torch.zeros_like(x)
    ab = torch.zeros_like(x)
    for i in range(3):
        for j in range(3):
            t = w[:, 0, i, j].view(1, d, 1, 1) * xp[:, :, i:i + H, j:j + W]
            pre = pre + t
            ab = ab + t.abs()
    return pre, ab


DW_CASES = [
    # (B, d, H, W, layout, path, where): layout packed / cmajor (the (d, B, H, W) hand-over of in_proj); path = the kernel
    # family the host code must pick (asserted below and against the recorded launch)
    (16, 192, 120, 160, "cmajor", "tiled", "s stage1 d_inner 192 at 120x160"),
    (16, 384, 60, 80, "cmajor", "plane", "s stage2 60x80"),
    (16, 768, 30, 40, "cmajor", "plane", "s stage3 30x40"),
    (16, 1536, 15, 20, "cmajor", "plane", "s stage4 15x20"),
    (8, 192, 120, 160, "packed", "tiled", "s decoder 120x160"),
    (8, 384, 30, 40, "packed", "plane", "s decoder 30x40"),
    (1, 2048, 23, 40, "cmajor", "plane", "b stage4 23x40"),
    (1, 512, 180, 320, "cmajor", "tiled", "b stage1 180x320"),
    (1, 256, 90, 160, "packed", "tiled", "b decoder 90x160"),
    # the 48 KiB switch, 2 (H + 2) ((W + 2) | 1) 4 bytes: 95 x 61 = 48888 B (last plane), 96 x 61 = 49392 B (first tiled);
    # tiled planes with W % 32 != 0 and H % 32 != 0 (partial column and row tiles of kTile = 32)
    (2, 8, 95, 61, "packed", "plane", "plane, 48888 B: last below 48 KiB"),
    (2, 8, 96, 61, "packed", "tiled", "tiled, 49392 B: first above 48 KiB, partial tiles"),
    (2, 6, 100, 70, "packed", "tiled", "tiled, partial column and row tiles"),
    (3, 5, 17, 33, "packed", "plane", "odd plane"), (2, 6, 33, 70, "packed", "plane", "plane, odd rows"),
]
for _B, _d, _H, _W, _l, _path, _w in DW_CASES:
    assert ("plane" if dw_plane(_H, _W) else "tiled") == _path, (_H, _W, _path)
    for _o in (1, 2):
        for _k in (("dw_fwd",), ("dw_bwd", False), ("dw_bwd", True)):      # backward: both values of the deterministic bit
            covers((_k[0], _path, _o, _l == "cmajor") + _k[1:], f"test_dwconv_silu_against_fp64[{_B}x{_d}x{_H}x{_W}-{_l}-o{_o}] ({_w})")


@pytest.mark.parametrize("orders", [2, 1], ids=["o2", "o1"])
@pytest.mark.parametrize("case", DW_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-{c[4]}" for c in DW_CASES])
def test_dwconv_silu_against_fp64(case, orders, record):
    """out2[:, 0] = silu(pre) row-major, out2[:, 1] = the same column-major; pre = nine shifted adds + bias (zero padding).
    pre: 10 terms, K = 10 + 6 (silu: exp2, rcp, 2 products), S = (sum|w x| + |b|) (1 + |pre|) -- silu' <= 1.1, and
    |silu(pre)| relative roundings.  Backward: gpre = (g0 + g1^T) silu'(pre): S_gpre = (|g0| + |g1|) (1.1 + |pre| S_pre-ish)
    taken as (|g0| + |g1|) (1.1 + S_pre); dx = nine shifted adds of w gpre: K = 9 + 24, S = conv^T(|w|, S_gpre).
    dweight[c] / dbias[c]: sums over B H W.  Plane kernel (one workgroup per plane): a thread serially over
    ceil(HW / 256) pixels, 6 wave levels, 3 adds of the 4 waves, B fp32 atomics.  Tiled kernel (one workgroup per 32 x 32
    tile, dwconv_silu_bwd1_kernel): 4 pixels per thread, 6 + 3 levels, B x tiles atomics, tiles = ceil(H / 32) ceil(W / 32).
    K = that serial depth + 24 (the error of gpre and the product), S = sum |S_gpre x| resp. sum S_gpre.  Negative controls: replicate padding; dbias without the last image."""
    from sigma_amd import _capi
    B, d, H, W, layout, path, _ = case
    assert ("plane" if dw_plane(H, W) else "tiled") == path
    lib = _capi.load()
    L = H * W
    if layout == "cmajor":
        xs = _rand(d, B, H, W, seed=11)
        x = xs.permute(1, 0, 2, 3)
        xbs, xcs = L, B * L
    else:
        x = _rand(B, d, H, W, seed=11)
        xbs, xcs = 0, 0
    w, b = _rand(d, 1, 3, 3, seed=12, scale=0.3), _rand(d, seed=13, scale=0.1)
    gout = _guarded((B, orders, d, L), L)
    p = _capi.DwConvParams()
    p.batch, p.channels, p.height, p.width, p.n_orders = B, d, H, W, orders
    p.x, p.weight, p.bias, p.out2 = x.data_ptr(), w.data_ptr(), b.data_ptr(), gout[1].data_ptr()
    p.x_batch_stride, p.x_channel_stride = xbs, xcs
    _capi.check(lib.sigma_dwconv3x3_silu_fwd(ctypes.byref(p), _stream()), "dwconv fwd")
    g2 = _rand(B, orders, d, L, seed=14)
    gdx = _guarded((B, d, H, W) if layout == "packed" else (d, B, H, W), L)
    dxv = gdx[1] if layout == "packed" else gdx[1].permute(1, 0, 2, 3)
    ggp = _guarded((B, d, H, W), L)                               # scratch of the tiled backward (bwd1 writes, bwd2 reads)
    gdw, gdb = _guarded((d, 9), 64), _guarded((d,), 64)
    gdw[1].zero_()
    gdb[1].zero_()
    dwb, dbb = gdw[1], gdb[1]
    p.g2, p.gpre, p.dweight, p.dbias, p.dx = g2.data_ptr(), ggp[1].data_ptr(), dwb.data_ptr(), dbb.data_ptr(), gdx[1].data_ptr()
    _capi.check(lib.sigma_dwconv3x3_silu_bwd(ctypes.byref(p), _stream()), "dwconv bwd")
    torch.cuda.synchronize()
    plane = "plane" if dw_plane(H, W) else "tiled"
    assert record == [("dw_fwd", plane, orders, layout == "cmajor"), ("dw_bwd", plane, orders, layout == "cmajor", False)], record
    _intact(gout, "out2")
    _intact(gdx, "dx")
    _intact(ggp, "gpre scratch")
    _intact(gdw, "dweight")
    _intact(gdb, "dbias")

    x64, w64, b64 = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    pre, ab = _dw_ref(x64, w64, b64)
    y = pre * torch.sigmoid(pre)
    o = [y.reshape(B, d, L)]
    if orders == 2:
        o.append(y.transpose(2, 3).reshape(B, d, L))
    out_ref = torch.stack(o, 1)
    out_ref.backward(g2.double())
    with torch.no_grad():
        S_pre = ab.detach() + b64.abs().view(1, d, 1, 1)
        S_y = S_pre * (1.1 + pre.abs())
        S_o = torch.stack([S_y.reshape(B, d, L)] + ([S_y.transpose(2, 3).reshape(B, d, L)] if orders == 2 else []), 1)
        check("dwconv", gout[1], out_ref.detach(), S_o, 16, "out2")
        ga = g2.double().abs()
        gsum = ga[:, 0].view(B, d, H, W) + (ga[:, 1].view(B, d, W, H).transpose(2, 3) if orders == 2 else 0.0)
        S_gpre = gsum * (1.1 + S_pre)
        S_dx = F.conv_transpose2d(S_gpre, w.double().abs(), padding=1, groups=d)
        check("dwconv", dxv, x64.grad, S_dx, 33, "dx")
        if plane == "tiled":
            Kr = 4 + 6 + 3 + B * -(-H // 32) * -(-W // 32) + 24
        else:
            Kr = -(-L // 256) + 6 + 3 + B + 24
        S_dw = torch.stack([(S_gpre * F.pad(x.double().abs(), (1, 1, 1, 1))[:, :, i:i + H, j:j + W]).sum((0, 2, 3))
                            for i in range(3) for j in range(3)], 1)
        check("dwconv", dwb, w64.grad.view(d, 9), S_dw, Kr, "dweight")
        check("dwconv", dbb, b64.grad, S_gpre.sum((0, 2, 3)), Kr, "dbias")
        # negative controls
        pre_r, _ = _dw_ref(x.double(), w.double(), b.double(), pad="replicate")
        yr = pre_r * torch.sigmoid(pre_r)
        wrong = torch.stack([yr.reshape(B, d, L)] + ([yr.transpose(2, 3).reshape(B, d, L)] if orders == 2 else []), 1)
        rejects(gout[1], wrong, S_o, 16, "replicate padding")
        if B > 1:
            sg = torch.sigmoid(pre.detach())
            gp = (g2.double()[:, 0].view(B, d, H, W) + (g2.double()[:, 1].view(B, d, W, H).transpose(2, 3) if orders == 2 else 0.0)) \
                * sg * (1 + pre.detach() * (1 - sg))
            rejects(dbb, gp[:-1].sum((0, 2, 3)), S_gpre.sum((0, 2, 3)), Kr, "dbias missing the last image")

    # deterministic mode (SIGMA_DWCONV_DETERMINISTIC): the same workgroup sums stored to one slot per (batch, tile), then
    # dwconv_reduce_kernel adds the slots of a channel in order -- the atomics' count of serial adds becomes the slot count:
    # K = the workgroup's depth + slots.  dweight / dbias / workspace stay NaN-filled: written, not added to
    p.flags = _capi.SIGMA_DWCONV_DETERMINISTIC
    slots = B * (1 if plane == "plane" else -(-H // 32) * -(-W // 32))
    nws = int(lib.sigma_dwconv3x3_silu_bwd_workspace_bytes(ctypes.byref(p)))
    assert nws == slots * d * 10 * 4
    gws = _guarded((nws // 4,), 64)
    gdx2 = _guarded(tuple(gdx[1].shape), L)
    ggp2 = _guarded((B, d, H, W), L)
    gdw2, gdb2 = _guarded((d, 9), 64), _guarded((d,), 64)
    p.gpre, p.dweight, p.dbias, p.dx = ggp2[1].data_ptr(), gdw2[1].data_ptr(), gdb2[1].data_ptr(), gdx2[1].data_ptr()
    p.workspace, p.workspace_bytes = gws[1].data_ptr(), nws
    _capi.check(lib.sigma_dwconv3x3_silu_bwd(ctypes.byref(p), _stream()), "dwconv bwd (deterministic)")
    torch.cuda.synchronize()
    assert record[2:] == [("dw_bwd", plane, orders, layout == "cmajor", True)], record
    for g_, w_ in ((gws, "workspace"), (gdx2, "dx"), (ggp2, "gpre scratch"), (gdw2, "dweight"), (gdb2, "dbias")):
        _intact(g_, w_ + " (deterministic)")
    assert torch.equal(gdx2[1], gdx[1]), "dx: deterministic mode changed it"
    if plane == "tiled":
        assert torch.equal(ggp2[1], ggp[1]), "gpre: deterministic mode changed it"
    else:                                                     # the whole-plane kernel keeps gpre in LDS
        assert bool(torch.isnan(ggp2[1]).all()) and bool(torch.isnan(ggp[1]).all())
    Kd = (4 + 6 + 3 if plane == "tiled" else -(-L // 256) + 6 + 3) + 24 + slots
    with torch.no_grad():
        check("dwconv det", gdw2[1], w64.grad.view(d, 9), S_dw, Kd, "dweight (deterministic)")
        check("dwconv det", gdb2[1], b64.grad, S_gpre.sum((0, 2, 3)), Kd, "dbias (deterministic)")
        if B > 1:
            rejects(gdb2[1], gp[:-1].sum((0, 2, 3)), S_gpre.sum((0, 2, 3)), Kd, "deterministic dbias missing the last image")


# ---------------------------------------------------------------------------------------------------------------------
# cross merge / split, transpose2d, pair_sum_add, bilinear x2

MERGE_CASES = [(16, 192, 120, 160, "s stage1"), (16, 1536, 15, 20, "s stage4"), (1, 2048, 23, 40, "b stage4 odd H"),
               (2, 12, 7, 5, "tiny odd")]
for _c in MERGE_CASES:
    covers(("merge",), f"test_cross_merge_split_against_fp64[{_c[0]}x{_c[1]}x{_c[2]}x{_c[3]}] ({_c[4]})")
    covers(("split",), f"test_cross_merge_split_against_fp64[{_c[0]}x{_c[1]}x{_c[2]}x{_c[3]}] ({_c[4]})")


@pytest.mark.parametrize("case", MERGE_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}" for c in MERGE_CASES])
def test_cross_merge_split_against_fp64(case, record):
    """merge: nhwc[b,h,w,c] = p0[hW+w] + p1[hW+w] + p2[wH+h] + p3[wH+h] (4 terms: K = 3, S = sum |terms|);
    split: planes2[b,0,c,hW+w] = planes2[b,1,c,wH+h] = nhwc[b,h,w,c] (copies: exact).  Negative control: the
    memory orders swapped (groups 0/1 read column-major, 2/3 row-major; H != W so the two differ)."""
    from sigma_amd import _capi
    B, d, H, W, _ = case
    L = H * W
    p4 = _rand(B, 4, d, L, seed=21)
    gm = _guarded((B, H, W, d), d)
    p = _capi.MergeParams()
    p.batch, p.channels, p.height, p.width = B, d, H, W
    p.planes4, p.nhwc = p4.data_ptr(), gm[1].data_ptr()
    _capi.check(_capi.load().sigma_cross_merge_nhwc(ctypes.byref(p), _stream()), "merge")
    nh = _rand(B, H, W, d, seed=22)
    gs = _guarded((B, 2, d, L), L)
    p.planes2, p.nhwc = gs[1].data_ptr(), nh.data_ptr()
    _capi.check(_capi.load().sigma_cross_split_nhwc(ctypes.byref(p), _stream()), "split")
    torch.cuda.synchronize()
    assert record == [("merge",), ("split",)]
    _intact(gm, "merge")
    _intact(gs, "split")
    q = p4.double()
    row = lambda t: t.view(B, d, H, W).permute(0, 2, 3, 1)
    col = lambda t: t.view(B, d, W, H).permute(0, 3, 2, 1)
    terms = [row(q[:, 0]), row(q[:, 1]), col(q[:, 2]), col(q[:, 3])]
    S = sum(t.abs() for t in terms)
    check("merge/split", gm[1], sum(terms), S, 3, "merge")
    rejects(gm[1], col(q[:, 0]) + col(q[:, 1]) + row(q[:, 2]) + row(q[:, 3]), S, 3, "merge with swapped orders")
    n = nh.permute(0, 3, 1, 2)
    want = torch.stack([n.reshape(B, d, L), n.transpose(2, 3).reshape(B, d, L)], 1)
    assert torch.equal(gs[1], want), "split"
    assert not torch.equal(gs[1], torch.stack([n.transpose(2, 3).reshape(B, d, L), n.reshape(B, d, L)], 1))


TR_CASES = [
    # (B, rows, cols, src_row_stride, dst_row_stride, where)
    (8, 19200, 96, 192, 19200, "decoder xz half -> (B, d, L)"),
    (16, 4800, 384, 768, 4800, "s stage2 x half of xz"),
    (16, 384, 4800, 4800, 768, "s stage2 dx into the x half"),
    (3, 37, 13, 29, 41, "odd strides"),
]
for _c in TR_CASES:
    covers(("transpose",), f"test_transpose2d_against_fp64[{_c[0]}x{_c[1]}x{_c[2]}] ({_c[5]})")


@pytest.mark.parametrize("case", TR_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in TR_CASES])
def test_transpose2d_against_fp64(case, record):
    """dst[b][c][r] = src[b][r][c] with free strides: a copy, exact.  Negative control: the untransposed copy."""
    from sigma_amd import _capi
    B, R, C, srs, drs, _ = case
    src = _rand(B, R, srs, seed=31)
    g = _guarded((B, C, drs), drs)
    p = _capi.TransposeParams()
    p.batch, p.rows, p.cols = B, R, C
    p.src, p.dst = src.data_ptr(), g[1].data_ptr()
    p.src_batch_stride, p.src_row_stride, p.dst_batch_stride, p.dst_row_stride = R * srs, srs, C * drs, drs
    _capi.check(_capi.load().sigma_transpose2d(ctypes.byref(p), _stream()), "transpose2d")
    torch.cuda.synchronize()
    assert record == [("transpose",)]
    _intact(g, "transpose")
    want = src[:, :, :C].transpose(1, 2)
    assert torch.equal(g[1][:, :, :R], want)
    assert bool(torch.isnan(g[1][:, :, R:]).all()), "transpose2d wrote the padding of the destination rows"
    if R != C:
        assert not torch.equal(g[1][:, :, :R].reshape(-1), src[:, :, :C].reshape(-1))


PS_CASES = [(16 * 192, 19200, 0, "s stage1 du pair (vec)"), (1 * 1024, 57600, 0, "b stage1 (vec)"),
            (64, 1001, 0, "inner % 4 != 0 (scalar)"), (64, 1000, 1, "4-byte offset views (scalar)")]
for _c in PS_CASES:
    covers(("pair_sum_add", "vec" if _c[1] % 4 == 0 and not _c[2] else "scalar"),
           f"test_pair_sum_add_against_fp64[{_c[0]}x{_c[1]}-off{_c[2]}] ({_c[3]})")


@pytest.mark.parametrize("case", PS_CASES, ids=[f"{c[0]}x{c[1]}-off{c[2]}" for c in PS_CASES])
def test_pair_sum_add_against_fp64(case, record):
    """acc[o] += src[2o] + src[2o+1]: 3 terms, two roundings (gamma_2 = 2u / (1 - 2u)): K = 3, S = sum |terms|.  Negative control: only one of the pair added."""
    from sigma_amd import _capi
    no, inner, off, _ = case
    src_buf = _rand(2 * no * inner + off, seed=41)
    src = src_buf[off:].view(no, 2, inner)
    ga = _guarded((no, inner), inner, offset=off)
    acc0 = _rand(no, inner, seed=42)
    ga[1].copy_(acc0)
    _capi.check(_capi.load().sigma_pair_sum_add(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(ga[1].data_ptr()), no, inner, _stream()),
                "pair_sum_add")
    torch.cuda.synchronize()
    assert record == [("pair_sum_add", "vec" if inner % 4 == 0 and not off else "scalar")], record
    _intact(ga, "pair_sum_add")
    s = src.double()
    S = acc0.double().abs() + s.abs().sum(1)
    check("pair_sum_add", ga[1], acc0.double() + s.sum(1), S, 3, "acc")
    rejects(ga[1], acc0.double() + s[:, 0], S, 3, "one of the pair")


def _up_ref(x, align_corners=False):
    """bilinear x2 of (B, H, W, C) from the align_corners=False weights: out[2i] = 3/4 x[i] + 1/4 x[i-1], out[2i+1] =
    3/4 x[i] + 1/4 x[i+1], indices clamped to the edge; separable (rows, then columns).  align_corners=True for the
    negative control."""
    def axis(t, dim):
        n = t.shape[dim]
        if align_corners:
            pos = torch.arange(2 * n, device=t.device, dtype=torch.float64) * (n - 1) / max(2 * n - 1, 1)
        else:
            pos = ((torch.arange(2 * n, device=t.device, dtype=torch.float64) + 0.5) / 2 - 0.5).clamp(min=0)
        i0 = pos.floor().long().clamp(max=n - 1)
        i1 = (i0 + 1).clamp(max=n - 1)
        f = (pos - i0).view(*([1] * dim), -1, *([1] * (t.dim() - dim - 1)))
        return t.index_select(dim, i0) * (1 - f) + t.index_select(dim, i1) * f
    return axis(axis(x, 1), 2)


UP_CASES = [(8, 120, 160, 96, "s decoder FinalUpsample 120x160x96"), (8, 60, 80, 192, "s decoder UpsampleExpand"),
            (1, 180, 320, 128, "b decoder 180x320"), (2, 7, 5, 12, "odd tiny")]
for _c in UP_CASES:
    for _m in ("fwd", "adjoint"):
        covers(("upsample", _m), f"test_upsample2x_against_fp64[{_c[0]}x{_c[1]}x{_c[2]}x{_c[3]}] ({_c[4]})")


@pytest.mark.parametrize("case", UP_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}" for c in UP_CASES])
def test_upsample2x_against_fp64(case, record):
    """forward: 4 weighted terms, K = 4 + 2, S = sum |w x|; adjoint (fp64 autograd of the reference): up to 16 weighted
    terms per input pixel, K = 16 + 2, S = the adjoint applied to |g|.  Negative control: align_corners=True."""
    from sigma_amd import _capi
    B, H, W, C, _ = case
    x = _rand(B, H, W, C, seed=51)
    go = _guarded((B, 2 * H, 2 * W, C), 2 * W * C)
    lib = _capi.load()
    _capi.check(lib.sigma_upsample2x_nhwc(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(go[1].data_ptr()), B, H, W, C, 0, _stream()), "up")
    g = _rand(B, 2 * H, 2 * W, C, seed=52)
    gi = _guarded((B, H, W, C), W * C)
    _capi.check(lib.sigma_upsample2x_nhwc(ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(gi[1].data_ptr()), B, H, W, C, 1, _stream()), "up adj")
    torch.cuda.synchronize()
    assert record == [("upsample", "fwd"), ("upsample", "adjoint")]
    _intact(go, "upsample")
    _intact(gi, "upsample adjoint")
    x64 = x.double().requires_grad_()
    y = _up_ref(x64)
    y.backward(g.double())
    with torch.no_grad():
        S = _up_ref(x.double().abs())
        check("upsample", go[1], y.detach(), S, 6, "forward")
        xa = x.double().abs().requires_grad_()
        with torch.enable_grad():
            _up_ref(xa).backward(g.double().abs())
        check("upsample", gi[1], x64.grad, xa.grad, 18, "adjoint")
        rejects(go[1], _up_ref(x.double(), align_corners=True), S, 6, "align_corners=True")


# ---------------------------------------------------------------------------------------------------------------------
# ChannelAttention plane ops, colscale_bwd

PLANE_CASES = [
    # (planes, hw, offset floats, where)
    (8 * 96, 19200, 0, "s decoder stage 120x160x96"), (8 * 384, 1200, 0, "s decoder 30x40x384"),
    (1 * 128, 57600, 0, "b decoder 180x320x128"), (40, 1001, 0, "hw % 4 != 0"), (40, 1000, 1, "4-byte offset views"),
]
for _c in PLANE_CASES:
    _v = "vec" if _c[1] % 4 == 0 and not _c[2] else "scalar"
    for _op in ("plane_pool", "plane_scale", "plane_dot", "plane_gate_bwd"):
        covers((_op, _v), f"test_plane_ops_against_fp64[{_c[0]}x{_c[1]}-off{_c[2]}] ({_c[3]})")


@pytest.mark.parametrize("case", PLANE_CASES, ids=[f"{c[0]}x{c[1]}-off{c[2]}" for c in PLANE_CASES])
def test_plane_ops_against_fp64(case, record):
    """pool: mean = sum / hw (a thread serially over ceil(hw / 256 (x4)), 8 levels: K = ceil(hw / 256) + 10, S = sum|x| / hw),
    max and count exact; scale: one product, one rounding (< u of the exact value), K = 2; dot: K = ceil(hw / 256) + 10, S = sum |a b|; gate_bwd: 3 terms with
    a division each, K = 5, S = |g s| + |dmean| / hw + |dmax| / count.  Ties of the max (count > 1) are planted.
    Negative controls: mean / dot without the last 4 elements of each plane."""
    from sigma_amd import _capi
    P, hw, off, _ = case
    lib = _capi.load()
    xb = _rand(P * hw + off, seed=61, mean=0.2)
    x = xb[off:].view(P, hw)
    mx0 = x.max(1).values
    x[:, 3], x[:, 5] = mx0, mx0                                    # every plane has a tied max
    gmean, gmax, gcnt = _guarded((P,), 1, offset=off), _guarded((P,), 1), _guarded((P,), 1)
    _capi.check(lib.sigma_plane_pool(ctypes.c_void_p(x.data_ptr()), P, hw, ctypes.c_void_p(gmean[1].data_ptr()),
                                     ctypes.c_void_p(gmax[1].data_ptr()), ctypes.c_void_p(gcnt[1].data_ptr()), _stream()), "pool")
    s = _rand(P, seed=62)
    gy = _guarded((P, hw), hw, offset=off)
    _capi.check(lib.sigma_plane_scale(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(gy[1].data_ptr()),
                                      P, hw, _stream()), "scale")
    gb = _rand(P * hw + off, seed=63)
    g = gb[off:].view(P, hw)
    gdot = _guarded((P,), 1)
    _capi.check(lib.sigma_plane_dot(ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(gdot[1].data_ptr()),
                                    P, hw, _stream()), "dot")
    dm, dmx = _rand(P, seed=64), _rand(P, seed=65)
    gdx = _guarded((P, hw), hw, offset=off)
    q = _capi.GateBwdParams()
    q.planes, q.hw = P, hw
    q.g, q.x, q.scale, q.dmean, q.dmax = g.data_ptr(), x.data_ptr(), s.data_ptr(), dm.data_ptr(), dmx.data_ptr()
    q.max, q.count, q.dx = gmax[1].data_ptr(), gcnt[1].data_ptr(), gdx[1].data_ptr()
    _capi.check(lib.sigma_plane_gate_bwd(ctypes.byref(q), _stream()), "gate_bwd")
    torch.cuda.synchronize()
    v = "vec" if hw % 4 == 0 and not off else "scalar"
    assert record == [("plane_pool", v), ("plane_scale", v), ("plane_dot", v), ("plane_gate_bwd", v)], record
    for gg, w in ((gmean, "mean"), (gmax, "max"), (gcnt, "count"), (gy, "scale"), (gdot, "dot"), (gdx, "gate_bwd")):
        _intact(gg, w)
    xd, gd = x.double(), g.double()
    Kr = -(-hw // 256) + 10
    S_mean = xd.abs().mean(1)
    check("plane ops", gmean[1], xd.mean(1), S_mean, Kr, "mean")
    mx = x.max(1).values
    assert torch.equal(gmax[1], mx)
    cnt = (x == mx[:, None]).sum(1).double()
    assert torch.equal(gcnt[1].double(), cnt) and bool((cnt >= 2).all())
    check("plane ops", gy[1], xd * s.double()[:, None], (xd * s.double()[:, None]).abs(), 2, "scale")
    S_dot = (gd * xd).abs().sum(1)
    check("plane ops", gdot[1], (gd * xd).sum(1), S_dot, Kr, "dot")
    hit = (x == mx[:, None]).double()
    ref = gd * s.double()[:, None] + dm.double()[:, None] / hw + hit * (dmx.double() / cnt)[:, None]
    S = (gd * s.double()[:, None]).abs() + dm.double().abs()[:, None] / hw + hit * (dmx.double().abs() / cnt)[:, None]
    check("plane ops", gdx[1], ref, S, 5, "gate_bwd")
    rejects(gmean[1], xd[:, :-4].sum(1) / hw, S_mean, Kr, "mean without the last 4 elements")
    rejects(gdot[1], (gd * xd)[:, :-4].sum(1), S_dot, Kr, "dot without the last 4 elements")


CS_CASES = [(8 * 19200, 96, "s decoder 120x160x96"), (8 * 4800, 192, "s decoder 60x80x192"), (8 * 1200, 384, "s decoder 30x40x384"),
            (8 * 300, 768, "s decoder 15x20x768"), (57600, 128, "b decoder 180x320x128"), (14400, 256, "b decoder 90x160x256"), (1001, 1024, "C = 1024"), (37, 4, "C = 4")]
for _c in CS_CASES:
    for _k in ("colscale_bwd", "colscale_bwd_ws"):
        covers((_k, 256 // (_c[1] // 4)), f"test_colscale_bwd_against_fp64[{_c[0]}x{_c[1]}] ({_c[2]})")


@pytest.mark.parametrize("case", CS_CASES, ids=[f"{c[0]}x{c[1]}" for c in CS_CASES])
def test_colscale_bwd_against_fp64(case, record):
    """dx = dy * s (one product, one rounding: K = 2); ds[c] += sum_rows dy x: a thread walks rows slot, slot + G slots, ... serially
    (ceil(rows / (G slots)) deep, G = min(512, ceil(rows / slots)) workgroups), the slots of a block meet in LDS (slots
    serial adds), G fp32 atomics: K = ceil(rows / (G slots)) + slots + G + 2, S = sum |dy x|.  Negative control: ds
    without the last partial row block (the rows of the last grid-stride step)."""
    from sigma_amd import _capi
    rows, C, _ = case
    slots = 256 // (C // 4)
    G = min(512, -(-rows // slots))
    x = _rand(rows, C, seed=71).abs()
    dy = 0.5 * x + _rand(rows, C, seed=72)
    s = _rand(C, seed=73)
    gdx = _guarded((rows, C), C)
    gds = _guarded((C,), C)
    gds[1].zero_()
    _capi.check(_capi.load().sigma_colscale_bwd(ctypes.c_void_p(dy.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(s.data_ptr()),
                                                ctypes.c_void_p(gdx[1].data_ptr()), ctypes.c_void_p(gds[1].data_ptr()), rows, C, _stream()),
                "colscale_bwd")
    torch.cuda.synchronize()
    assert record == [("colscale_bwd", slots)]
    _intact(gdx, "dx")
    _intact(gds, "ds")
    dd, xd = dy.double(), x.double()
    check("colscale_bwd", gdx[1], dd * s.double(), (dd * s.double()).abs(), 2, "dx")
    K = -(-rows // (G * slots)) + slots + G + 2
    S = (dd * xd).abs().sum(0)
    check("colscale_bwd", gds[1], (dd * xd).sum(0), S, K, "ds")
    if rows > G * slots:
        tail = rows % (G * slots) or G * slots
        rejects(gds[1], (dd * xd)[:rows - tail].sum(0), S, K, "ds missing the last row block")

    # deterministic form (sigma_colscale_bwd_ws): the G block sums are stored to workspace rows, then colscale_reduce_kernel
    # adds them in a fixed order (thread y of 16 adds rows y, y + 16, ..., then the 16 partials in order):
    # K = ceil(rows / (G slots)) + slots + ceil(G / 16) + 16 + 2.  ds and the workspace stay NaN-filled: ds is written
    n = int(_capi.load().sigma_colscale_bwd_workspace_bytes(rows, C))
    assert n == G * C * 4
    gws, gdx2, gds2 = _guarded((n // 4,), C), _guarded((rows, C), C), _guarded((C,), C)
    _capi.check(_capi.load().sigma_colscale_bwd_ws(ctypes.c_void_p(dy.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(s.data_ptr()),
                                                   ctypes.c_void_p(gdx2[1].data_ptr()), ctypes.c_void_p(gds2[1].data_ptr()), rows, C,
                                                   ctypes.c_void_p(gws[1].data_ptr()), n, _stream()), "colscale_bwd_ws")
    torch.cuda.synchronize()
    assert record == [("colscale_bwd", slots), ("colscale_bwd_ws", slots)], record
    for g_, w_ in ((gws, "workspace"), (gdx2, "dx"), (gds2, "ds")):
        _intact(g_, w_ + " (deterministic)")
    assert torch.equal(gdx2[1], gdx[1]), "dx: the deterministic form changed it"
    Kd = -(-rows // (G * slots)) + slots + -(-G // 16) + 16 + 2
    check("colscale det", gds2[1], (dd * xd).sum(0), S, Kd, "ds (deterministic)")
    cut = rows - (rows % (G * slots) or G * slots) if rows > G * slots else rows - 1
    rejects(gds2[1], (dd * xd)[:cut].sum(0), S, Kd, "deterministic ds missing the last row block (or row)")


# ---------------------------------------------------------------------------------------------------------------------
# softmax cross entropy

CE_CASES = [(8 * 480 * 640, 40, "s NYUDepth 40 classes 480x640 (batch 8)"), (720 * 1280, 8, "720x1280 rows, 8 classes"),
            (20000, 64, "64 classes (reg, last)"), (20000, 68, "68 classes (generic)"), (3001, 4, "4 classes, odd rows"),
            (4096, 152, "152 classes (generic)")]
for _c in CE_CASES:
    for _ph in ("fwd", "bwd"):
        covers(("ce_" + _ph, "reg" if _c[1] // 4 <= 16 else "generic"), f"test_softmax_ce_against_fp64[{_c[0]}x{_c[1]}] ({_c[2]})")


@pytest.mark.parametrize("case", CE_CASES, ids=[f"{c[0]}x{c[1]}" for c in CE_CASES])
def test_softmax_ce_against_fp64(case, record):
    """lse[r] = logsumexp(logits[r]) (fp64); loss = sum over labelled rows (lse - logit[label]) / count; ~10 % of the
    pixels carry ignore_index (255).  lse: max exact, a sum of nc exps (exp2 within 2 ulp): K = nc + 8, S = |lse| + 1.
    partial[:, 0] (per-block loss sums) summed in fp64: every thread serially over ceil(rows / 256 K_B) rows, 8 levels in
    the block: K = ceil(rows / (256 x 1024)) + 8 + nc + 8, S = sum over labelled rows (|lse| + 1 + |logit[label]|);
    partial[:, 1] (counts): exact.  dlogits = scale (softmax - onehot), 0 on ignored rows: K = nc + 16,
    S = scale (p (|x| + |lse| + 1) + onehot).  Negative control: ignored pixels counted as class 0."""
    from sigma_amd import _capi
    rows, nc, _ = case
    lib = _capi.load()
    logits = _rand(rows, nc, seed=81, scale=3.0)
    g = torch.Generator(device=DEV).manual_seed(82)
    lab = torch.randint(0, nc, (rows,), generator=g, device=DEV)
    lab[torch.rand(rows, generator=g, device=DEV) < 0.1] = 255
    glse = _guarded((rows,), 64)
    part = _guarded((_capi.SIGMA_CE_BLOCKS, 2), 2)
    _capi.check(lib.sigma_softmax_ce_fwd(ctypes.c_void_p(logits.data_ptr()), ctypes.c_void_p(lab.data_ptr()), rows, nc, 255,
                                         ctypes.c_void_p(glse[1].data_ptr()), ctypes.c_void_p(part[1].data_ptr()), _stream()), "ce fwd")
    torch.cuda.synchronize()
    valid = lab != 255
    cnt = float(valid.sum())
    scale = torch.tensor([0.7 / cnt], device=DEV)
    gdl = _guarded((rows, nc), nc)
    _capi.check(lib.sigma_softmax_ce_bwd(ctypes.c_void_p(logits.data_ptr()), ctypes.c_void_p(lab.data_ptr()), ctypes.c_void_p(glse[1].data_ptr()),
                                         ctypes.c_void_p(scale.data_ptr()), rows, nc, 255, ctypes.c_void_p(gdl[1].data_ptr()), _stream()), "ce bwd")
    torch.cuda.synchronize()
    path = "reg" if nc // 4 <= 16 else "generic"
    assert record == [("ce_fwd", path), ("ce_bwd", path)]
    for gg, w in ((glse, "lse"), (part, "partial"), (gdl, "dlogits")):
        _intact(gg, w)
    x = logits.double()
    lse = torch.logsumexp(x, 1)
    S_lse = lse.abs() + 1.0
    check("cross entropy", glse[1][valid], lse[valid], S_lse[valid], nc + 8, "lse")
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    xl = x.gather(1, safe[:, None])[:, 0]
    loss_rows = torch.where(valid, lse - xl, torch.zeros_like(lse))
    K = -(-rows // (256 * _capi.SIGMA_CE_BLOCKS)) + 8 + nc + 8
    S_loss = torch.where(valid, S_lse + xl.abs(), torch.zeros_like(lse)).sum()
    got_sum = part[1][:, 0].double().sum()
    check("cross entropy", got_sum.view(1), loss_rows.sum().view(1), S_loss.view(1), K, "loss sum")
    assert float(part[1][:, 1].double().sum()) == cnt
    p = torch.softmax(x, 1)
    oh = F.one_hot(safe, nc).double()
    sc = float(scale)
    ref = torch.where(valid[:, None], sc * (p - oh), torch.zeros_like(p))
    S = torch.where(valid[:, None], sc * (p * (x.abs() + lse.abs()[:, None] + 1.0) + oh), torch.zeros_like(p))
    check("cross entropy", gdl[1], ref, S, nc + 16, "dlogits")
    rejects(gdl[1], sc * (p - oh), S, nc + 16, "ignored pixels counted as class 0")
    wrong_sum = (lse - xl).sum()
    rejects(got_sum.view(1), wrong_sum.view(1), S_loss.view(1), K, "ignored pixels in the loss sum")


# ---------------------------------------------------------------------------------------------------------------------
# GEMM paths of the two models -> the fp64 case in tests/test_gemm_gpu.py that runs them at a real shape
_G = ("gemm",)
# key -> (test function of tests/test_gemm_gpu.py, its arguments): test_gemm_cases_launch_their_census_keys RUNS each case
# under the recorder and asserts that it launches the key; the census then only needs the key to be here
GEMM_CASES = {
    # (form, pieces, batch > 1, a_mod, c_mod summed, k_slices, t_cols, residuals, bias, accumulate, tile width, epilogue, stage);
    # tile width and epilogue kind are sigma_gemm_plan's report: a dispatch change that moves a model launch to another kernel
    # variant or epilogue changes its key
    _G + ("nt", 2, False, False, False, False, False, 0, False, False, 128, "rows", "own"): ("test_gemm_nt_against_fp64", ((19200, 384, 1536), False)),
    _G + ("nt", 2, False, False, False, False, False, 0, True, False, 128, "rows", "own"): ("test_gemm_nt_against_fp64", ((19200, 384, 1536), True)),
    _G + ("nt", 2, False, False, False, False, False, 1, False, False, 128, "rows", "own"): ("test_linear_with_the_residual_added_in_the_kernel",
                                                                               ((19200, 768, 384),)),
    _G + ("nt", 2, False, False, False, False, True, 0, False, False, 128, "transposed", "own"): ("test_in_proj_with_channel_major_x_half_against_fp64",
                                                                              ((2, 30, 40, 384, 768), False)),
    _G + ("nt", 2, True, False, True, False, False, 0, False, False, 96, "rows", "two-stage"): ("test_shared_outputs_sum_in_two_stages", ()),
    _G + ("nn", 2, False, False, False, False, False, 0, False, False, 128, "rows", "own"): ("test_gemm_nn_against_fp64", ((19200, 1536, 384),)),
    _G + ("nn", 2, False, False, False, True, False, 0, False, False, 128, "rows", "two-stage"):
        ("test_gemm_nn_with_a_sliced_reduction_against_fp64", ((768, 19200, 384),)),
    _G + ("nn", 2, True, True, False, False, False, 0, False, False, 96, "rows", "own"):
        ("test_stacked_projections_of_the_scan_core_against_fp64", ((2, 768, 56, 24, 1200),)),
    _G + ("nn", 2, True, True, False, False, False, 2, False, False, 96, "rows", "own"):
        ("test_stacked_projections_of_the_scan_core_against_fp64", ((2, 768, 56, 24, 1200),)),
    _G + ("nn", 2, True, False, False, False, False, 0, False, False, 128, "rows", "own"):
        ("test_stacked_projections_of_the_scan_core_against_fp64", ((1, 1536, 80, 48, 300),)),
    _G + ("nn", 2, True, False, False, False, False, 2, False, False, 128, "rows", "own"):
        ("test_stacked_projections_of_the_scan_core_against_fp64", ((1, 1536, 80, 48, 300),)),
    _G + ("tn", 2, False, False, False, False, False, 0, False, False, 128, "rows", "own"): ("test_gemm_tn_against_fp64", ((300, 1536, 768),)),
    _G + ("tn", 2, False, False, False, False, False, 0, False, True, 128, "rows", "own"): ("test_gemm_tn_against_fp64", ((300, 1536, 768),)),
    _G + ("tn", 2, False, False, False, False, False, 0, False, False, 128, "rows", "two-stage"): ("test_gemm_tn_against_fp64", ((19200, 1536, 384),)),
    _G + ("tn", 2, False, False, False, False, False, 0, False, True, 128, "rows", "two-stage"): ("test_gemm_tn_against_fp64", ((19200, 1536, 384),)),
}
GEMM_COVERED = {k: f"tests/test_gemm_gpu.py::{fn}{list(args)}" for k, (fn, args) in GEMM_CASES.items()}
_GEMM_RUNS = sorted({(fn, args) for fn, args in GEMM_CASES.values()}, key=repr)


@pytest.mark.parametrize("run", _GEMM_RUNS, ids=[f"{fn}-{i}" for i, (fn, _) in enumerate(_GEMM_RUNS)])
def test_gemm_cases_launch_their_census_keys(run, record):
    """runs the fp64 GEMM case named in GEMM_CASES under the recorder: it must pass AND launch every key mapped to it"""
    import tests.test_gemm_gpu as tg
    fn, args = run
    getattr(tg, fn)(*args)
    torch.cuda.synchronize()
    want = {k for k, v in GEMM_CASES.items() if v == run}
    assert want <= set(record), f"{fn}{args} does not launch {want - set(record)}"


def _gemm_exact_cases():
    """census key -> the exact case of tests/test_gemm_exact_gpu.py that launches it (planned on the host, as
    tests/test_gemm_exact_cpu.py does): where a key has an exact case, it is the one named"""
    from sigma_amd import _capi
    from tests.test_gemm_exact_gpu import CASES
    lib = _capi.load()
    exact = {}
    for c in CASES:
        p = c.params(c.FAKE)
        need = int(lib.sigma_gemm_workspace_bytes(ctypes.byref(p), _capi.GEMM_FORMS[c.form]))
        if need > 0 and c.ws != "none":
            p.workspace, p.workspace_bytes = c.FAKE["ws"], need - (1 if c.ws == "short" else 0)
        exact.setdefault(launch_key(lib, f"sigma_gemm_{c.form}_split3", (ctypes.byref(p), None)),
                         f"tests/test_gemm_exact_gpu.py::test_exact_case[{c.name}]")
    return exact


GEMM_EXACT = _gemm_exact_cases()
COVERED.update(GEMM_EXACT)
for _k, _v in GEMM_COVERED.items():            # the fp64 case at the real shape is named as well
    COVERED[_k] = f"{COVERED[_k]} + {_v}" if _k in COVERED else _v


# ---------------------------------------------------------------------------------------------------------------------
# scan launches: key -> the oracle / C-ABI case that runs it; each case asserts at run time that it launches its keys
# (scan_case_keys), so registering them here re-runs nothing
def _scan_covered():
    from tests.test_deterministic_gpu import FAMILIES
    from tests.test_scan_gpu import FULL_LAUNCHES, LONG_SHAPES
    for c in FULL_LAUNCHES:
        for k in scan_case_keys(*c, det=(False, True)):
            covers(k, f"tests/test_scan_gpu.py::test_full_size_step_launches_against_oracle[{c}]")
    for c in LONG_SHAPES:
        for pitch in LONG_PITCHES:
            for k in scan_case_keys(*c, pitch):
                covers(k, f"tests/test_scan_gpu.py::test_long_sequences_of_the_720x1280_configuration[{c}-{pitch}]")
    for c in FAMILIES:
        for k in scan_case_keys(*c[:8], IO_DTYPES[c[8]], det=(False, True)):
            covers(k, f"tests/test_deterministic_gpu.py::test_every_family_writes_all_row_gradients[{c}]")


def _scan_fp64_cases():
    """the scan keys that have a case under the derived fp64 bound (tests/test_scan_fp64_gpu.py): key -> that case"""
    from tests.test_scan_fp64_gpu import CASES
    tight = {}
    for c in CASES:
        for k in scan_case_keys(*c[1:9], IO_DTYPES[c[9]], det=(False, True)):
            tight.setdefault(k, f"tests/test_scan_fp64_gpu.py::test_every_family_on_every_regime[{c[0]}-*]")
    return tight


IO_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
LONG_PITCHES = (0, 640, 320, 160)
COVERED.update(_scan_fp64_cases())          # first: where a scan key has the tighter test, it is the one named
_scan_covered()


def _census(model_name, H, W, batch, classes, record):
    from tests.model_utils import build_model, fill
    model = build_model(model_name, classes, H, W).cuda().train()
    rgb, x, label = fill.make_inputs(batch, H, W, classes, seed=3)
    del record[:]
    loss = model(rgb.cuda(), x.cuda(), label.cuda())
    loss.backward()
    torch.cuda.synchronize()
    keys = sorted({k for k in record if k is not None}, key=repr)
    del model
    torch.cuda.empty_cache()
    return keys


CENSUS_MODELS = (("sigma_small", 480, 640, 2, 40), ("sigma_base", 720, 1280, 1, 5))


def test_census_of_both_models_is_covered(record):
    """one forward + backward of sigma_small 480x640 (batch 2) and sigma_base 720x1280 (batch 1): every stream-kernel /
    GEMM / scan path they take must be a key of COVERED"""
    seen = {}
    for name, H, W, batch, classes in CENSUS_MODELS:
        seen[name] = _census(name, H, W, batch, classes, record)
    missing = []
    for name, keys in seen.items():
        print(f"\ncensus {name}: {len(keys)} keys")
        for k in keys:
            print("  ", k, "->", COVERED.get(k, "NOT COVERED"))
            if k not in COVERED:
                missing.append((name, k))
    assert not missing, f"paths without an fp64 case: {missing}"


# project paths of the deterministic step that keep a float atomic on purpose: key -> the documented reason (none)
NONDETERMINISTIC_ALLOWED: dict = {}


def nondeterministic(key) -> bool:
    """a key whose launch sums with float atomics: a GEMM stage "atomic", a scan / dwconv backward without the
    deterministic bit, the atomic colscale backward"""
    if key[0] == "gemm":
        return key[-1] == "atomic"
    if key[0] in ("scan_bwd", "dw_bwd"):
        return key[-1] is not True if key[0] == "dw_bwd" else len(key) < 3 or key[2] is not True
    return key[0] == "colscale_bwd"


def test_census_of_the_deterministic_step():
    """the census of test_census_of_both_models_is_covered under torch's flag (warn_only: torch's own refusals warn), in a
    child process (tests/deterministic_census_worker.py; the flag and CUBLAS_WORKSPACE_CONFIG stay out of this one):
    (a) every key is in COVERED, (b) no project path sums with float atomics unless NONDETERMINISTIC_ALLOWED says why"""
    import ast
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CUBLAS_WORKSPACE_CONFIG=":4096:8")
    r = subprocess.run([sys.executable, "-m", "tests.deterministic_census_worker"], cwd=root, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, f"worker exit {r.returncode}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    assert "[deterministic_census_worker] done" in r.stdout
    seen = {}
    for line in r.stdout.splitlines():
        if line.startswith("[census] "):
            name, keys = line[9:].split(" ", 1)
            seen[name] = ast.literal_eval(keys)
    assert sorted(seen) == sorted(m[0] for m in CENSUS_MODELS), r.stdout[-4000:]
    missing, atomic = [], []
    for name, keys in seen.items():
        print(f"\ndeterministic census {name}: {len(keys)} keys")
        for k in keys:
            print("  ", k, "->", COVERED.get(k, "NOT COVERED"), "(NON-DETERMINISTIC)" if nondeterministic(k) else "")
            if k not in COVERED:
                missing.append((name, k))
            if nondeterministic(k) and k not in NONDETERMINISTIC_ALLOWED:
                atomic.append((name, k))
    assert not missing, f"paths without an fp64 case: {missing}"
    assert not atomic, f"float-atomic paths in the deterministic step: {atomic}"


def test_zz_report_worst_ratios():
    """prints the worst error / bound ratio of each family (the cases above asserted <= 1)"""
    print("\nworst |err| / (K u S) per family:")
    for fam, r in sorted(WORST.items()):
        print(f"   {fam:15s} {r:.3g}")
