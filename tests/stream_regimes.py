"""Edge shapes and named value regimes for the stream kernels (csrc/layernorm.hip, merge.hip, upsample.hip and the plane /
colscale kernels of pointwise.hip, dwconv.hip), fp64 twins that survive non-finite inputs, fp32 emulations of the LayerNorm
and depthwise-conv kernels and the wrong variants every regime must reject.  Shared by tests/test_stream_regimes_cpu.py
(the emulation under the bounds and the wrong variants rejected, so that the GPU tests cannot pass vacuously) and
tests/test_stream_regimes_gpu.py (the kernels through the C ABI).  Every function works on CPU or device tensors alike; nothing here needs a GPU.

Bounds.  The existing ones of tests/test_stream_fp64_gpu.py (|got - ref| <= K u S, u = 2^-24), restated in ``ln_twin`` in
closed form (no autograd: a poisoned row must stay a poisoned row, and autograd of x.var() spreads 0 * NaN).  K and S are
those of test_layernorm_against_fp64.  Three additions, each in S and each switched on only by the regimes that need it:

Second-order term of rstd (``second_order``; the ``offset`` regime).  The two-pass variance taken around a computed mean
mu^ = mu + delta is  mean((x - mu^)^2) = var + delta^2  exactly: the mean's error enters the variance in second order, which
the existing S_rstd = r drops.  |delta| <= D = (d + 2) u mean|x| (the existing bound of the mean), so
    |r^ - r| <= (d + 12) u r  +  r^3 D^2 / 2 .
At mean 0.3 the term is 1e-10 of r; at mean 1e4 on sd 0.02 it is the whole error (D = 7e-3 against sd 0.02).  y, dx and dz
need nothing: their S carries r mean|x| (and its square), the first-order effect of delta, which is far larger.

Argument error of the sigmoid (``saturated``; gates of +-20 ... +-200).  sigmoid_f(z) = rcp(1 + exp2(-z log2 e)): the
product -z log2(e) rounds once and the constant is rounded, an absolute error of <= 2 u |z| log2(e) of the argument, which
exp2 turns into a relative error 2 |z| u of e = exp(-z), and  d sigma / sigma = -(1 - sigma) de / e :
    rho = 2 |z| (1 - sigma(z))  (in units of u)  relative on sigma, hence on silu(z) = z sigma(z).
The roundings are relative to sigma as well: exp2 is within 2 ulp of e^, the sum 1 + e^ rounds to nearest (relative u / 2
of the sum; for e^ < u its error is also below e^ itself, since 1 is representable), and rcp adds one ulp of the
quotient unless the sum is exactly 1.  Relative to sigma that is at most 3 u, and at most 6 e once e is tiny (a large
positive gate, where sigma^ is exactly 1).  So  |s^ - sigma| <= u sigma (rho + min(6 e / u, 3)) =: u ds , a RELATIVE error
of sigma on both sides: at z = -20 it is 43 u of sigma = 2e-9, not an absolute 3 u.  The existing bounds carry "4 ulp of
silu" relative to |silu(z)|; what they do not carry is the part that grows with |z|:
    y:   S += |n rs| |z| ds / K = |y| (rho + ...) / K               (n = xhat gamma + beta)
    dx, dgamma, dbeta: the same error of gpre = dy silu(z) rs, pushed through the sums of their S
    dz = dy rs n sigma (1 + z (1 - sigma)):  both factors move with s^:  S += |dy rs n| ds (1 + |z|) / K .
The gate of the LayerNorm is an input, exact, so these bounds stay relative to the value down to fp32's normal range and a
sigma flushed to zero at z = -20 is rejected (``flushed``).  The pre-activation of the depthwise conv is computed: its own
error, (nine terms) u S_pre, times silu' <= 1.1 is what the existing S_out2 carries, and that dominates at any saturated
value -- there the term is added for completeness and the clamp is seen on the positive side alone.

Underflow (``saturated``).  Below fp32's normal range a result may come back subnormal or be flushed to zero:
sigma(-88) = 6e-39, and exp2 overflows from z = -88.8 on, so s^ = 0 where sigma = 1e-39 ... 1e-87.  An absolute error of
<= 2^-126 of s^ and of each product formed from it: tests/loss_regimes.underflow_S with f = the factor s^ is multiplied by.
"""
from __future__ import annotations

import torch

from tests.loss_regimes import underflow_S
from tests.test_dwconv_shapes_gpu import _two_orders
from tests.test_stream_fp64_gpu import _dw_ref, ln_nv

U = 2.0 ** -24
EPS = 1e-5
LOG2E = 1.4426950408889634
NAN, INF = float("nan"), float("inf")


def ratio(got, ref, S, K):
    """max |got - ref| / (K u S), as ``_ratio`` of tests/test_stream_fp64_gpu.py; NaN where got is not finite"""
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return float(((got.double() - ref).abs() / (K * U * S + 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------
# Part A: the edge-shape tables

LN_VARIANTS = ("plain", "dx_add", "gated", "gated_rs")
LN_SMALL = [(r, c) for r in (1, 2, 3, 4, 5, 7) for c in (4, 8, 252, 256, 260)]
# every wave walks several rows with an odd tail; NV = 1 (a single live lane), NV = 2 (prefetch chain), NV = 4 (none)
LN_WALK = [(20001, 4, "gated_rs"), (20001, 260, "gated"), (20001, 772, "dx_add"), (20001, 260, "plain")]
# (samples, rows per sample, C): the per-wave carry of the row factor takes several steps (1200 and 4001 rows per sample
# against up to 8192 waves), none (7 rows per sample, one row per wave) and one sample per row
LN_FACTOR = [(16, 1200, 96), (5, 4001, 192), (3, 7, 256), (16, 1, 384)]
FACTORS = (1.0 / 0.9, 1.0, 0.0, 1.0 / 0.5)


_A, _B = 1.0 / 0.9, 1.0 / 0.5
# per sample count: distinct neighbours from {0, 1, 1/0.9, 1/0.5}, one zero in the middle, the last sample nonzero
_FACTOR_TABLE = {
    1: [_A], 2: [0.0, 1.0], 3: [_A, 0.0, _B], 4: [_A, 0.0, 1.0, _B], 5: [_A, 1.0, 0.0, _B, _A], 7: [_A, 1.0, _A, 0.0, _A, 1.0, _B],
    16: [_A, 1.0, _A, _B, _A, 1.0, _A, 0.0, _A, 1.0, _A, _B, _A, 1.0, _A, _B],
}


def factors(nsamp):
    return list(_FACTOR_TABLE[nsamp])


# cross merge / split: (B, d, H, W) and the grid B ceil(H / 16) ceil(W / 16) ceil(d / 32) of each.  The issue's sets give
# the grids 1, 2, 3, 4, 6, 9, 12, 18, 27 (residues 1, 2, 3, 4, 6 mod 8, six of them below 8); the four cases after them
# add the residues 5, 7 and 0 and a grid of 36 (xcd_logical_block deals the ids to 8 XCDs)
_HW = [(1, 1), (1, 17), (17, 1), (15, 17), (16, 16), (33, 16)]
MERGE_CASES = [(B, d, H, W) for B in (1, 3) for d in (1, 31, 32, 33, 65) for H, W in _HW] + \
              [(5, 1, 1, 1), (7, 32, 16, 16), (1, 33, 17, 17), (2, 65, 33, 17)]      # grids 5, 7, 8, 36


def merge_grid(B, d, H, W):
    return B * -(-H // 16) * -(-W // 16) * -(-d // 32)


TR_CASES = [(B, R, C, pad) for B in (1, 3) for R in (1, 31, 32, 33) for C in (1, 31, 32, 33) for pad in (0, 5)]
# (n_outer, inner, offset floats)
PS_CASES = [(no, inner, off) for inner in (1, 3, 4, 5, 4096, 4100) for no in (1, 2) for off in (0, 1)] + \
           [(no, 4, off) for no in (65535, 65536, 70001) for off in (0, 1)]
UP_CASES = [(1, 1, 1, 4), (1, 1, 2, 4), (1, 2, 1, 4), (2, 1, 7, 8), (1, 3, 3, 4), (1, 2, 5, 12)]
PLANE_HW = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
PLANE_CASES = [(P, hw, off) for hw in PLANE_HW for P in (1, 3) for off in (0, 1)]
CS_C = (4, 8, 12, 96, 100, 516, 1020, 1024)


def cs_rows(C):
    slots = 256 // (C // 4)
    return [r for r in dict.fromkeys((1, slots - 1, slots, slots + 1, 512 * slots + 1)) if r > 0]


def second_tie(hw):
    """the position of the second planted maximum (the first is element 0): another wave of the 256 threads wherever the
    plane has one -- thread i reads elements i, i + 256, ... (scalar) or the float4s i, i + 256, ... (vec)"""
    return hw - 1 if hw <= 256 else (200 if hw <= 600 else 600)


def plane_inputs(P, hw, kinds, seed, device="cpu"):
    """(P, hw) fp32 planes, plane p of kind kinds[p % len(kinds)]: "tied" two maxima (element 0 and ``second_tie``),
    "constant" (count == hw), "last" the unique maximum in the last element, "neg_inf" all -inf, "pos_inf" two +inf"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, hw, generator=g) + 0.2
    for p in range(P):
        k = kinds[p % len(kinds)]
        top = float(x[p].max()) + 1.0
        if k == "tied":
            x[p, 0] = x[p, second_tie(hw)] = top
        elif k == "constant":
            x[p] = 0.75 * (p + 1)
        elif k == "last":
            x[p, hw - 1] = top
        elif k == "neg_inf":
            x[p] = -INF
        elif k == "pos_inf":
            x[p, 0] = x[p, second_tie(hw)] = INF
    return x.to(device)


# ---------------------------------------------------------------------------------------------------------------------
# Part B: LayerNorm regimes

LN_REGIMES = ("offset", "constant", "wide", "outlier")
LN_REGIME_CASES = [(300, 96), (300, 260), (300, 1024), (9003, 96)]      # the last: several rows per wave (8192 waves at most)
OFFSETS = (10.0, -10.0, 1e3, -1e3, 1e4)
CONSTANTS = (0.0, -0.0, 1.0, -3.0, 1e4, 1e-30)
GATES = (20.0, 60.0, 88.0, 90.0, 104.0, 200.0)


def ln_regime(name, rows, C, seed):
    """x (rows, C) fp32 on the CPU.  offset: a row mean of +-10, +-1e3, 1e4 on sd 0.02; constant: whole rows of 0, -0.0, 1,
    -3, 1e4, 1e-30; wide: (0.3 + randn) 2^e, e from -40 to 40 over the rows; outlier: one element of 1e4 per row"""
    g = torch.Generator().manual_seed(seed)
    r = torch.arange(rows)
    if name == "offset":
        return torch.tensor(OFFSETS)[r % len(OFFSETS)][:, None] + 0.02 * torch.randn(rows, C, generator=g)
    if name == "constant":
        return torch.tensor(CONSTANTS)[r % len(CONSTANTS)][:, None].expand(rows, C).contiguous()
    if name == "wide":
        e = torch.linspace(-40, 40, min(rows, 81)).round()[r % min(rows, 81)]
        return (0.3 + torch.randn(rows, C, generator=g)) * (2.0 ** e)[:, None]
    if name == "outlier":
        x = torch.randn(rows, C, generator=g)
        x[r, (7 * r + 3) % C] = 1e4
        return x
    if name == "base":
        return 0.3 + 0.02 * torch.randn(rows, C, generator=g)
    raise ValueError(name)


def saturated_gate(rows, C, seed):
    """gate values of +-20, +-60, +-88, +-90, +-104, +-200 on every fourth column (the sign alternates with the row), N(0, 1)
    elsewhere: every row keeps ordinary gates, so its sums are not all underflow"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, C, generator=g)
    r, c = torch.arange(rows)[:, None], torch.arange(C)[None, :]
    val = torch.tensor(GATES)[(r + c // 4) % len(GATES)] * torch.where((r + c // 4 // len(GATES)) % 2 == 0, 1.0, -1.0)
    return torch.where(c % 4 == 1, val, z)


def ln_params(C, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return ((1.0 + 0.5 * torch.randn(C, generator=g)).to(device), (0.1 * torch.randn(C, generator=g)).to(device))


def ln_case(rows, C, variant, regime, seed=900, gate="normal"):
    """fp32 CPU inputs of a LayerNorm case: x of the regime, gamma, beta, the gate, the per-row factor, dy, dx_add"""
    gated, scaled, dxa = variant.startswith("gated"), variant == "gated_rs", variant == "dx_add"
    g = torch.Generator().manual_seed(seed + 1)
    x = ln_regime(regime, rows, C, seed)
    gamma, beta = ln_params(C, seed + 2)
    z = (saturated_gate(rows, C, seed + 3) if gate == "saturated" else torch.randn(rows, C, generator=g)) if gated else None
    assert rows % 3 == 0 or not scaled                   # three samples of rows / 3 rows each
    rs = torch.tensor(factors(3)).repeat_interleave(rows // 3) if scaled else None
    dy = torch.randn(rows, C, generator=g)
    dadd = torch.randn(rows, C, generator=g) if dxa else None
    return x, gamma, beta, z, rs, dy, dadd


def ln_K(rows, C, G):
    """the constants of test_layernorm_against_fp64; G = workgroups of the backward (its partial rows)"""
    d = 4 * ln_nv(C) + 6
    G = max(G, 1)
    Kc = -(-rows // (4 * G)) + -(-G // 16) + 20
    return dict(d=d, y=d + 12, mean=d + 2, rstd=d + 12, dx=2 * d + 16, dgamma=Kc + d + 12, dbeta=Kc, dz=d + 20)


def _sig_terms(z):
    """sigma(z), silu(z) and ds of the module docstring (in units of u), fp64"""
    sg = torch.sigmoid(z)
    e = torch.exp(-z.clamp(-700, 700))
    rho = 2.0 * z.abs() * (1.0 - sg)
    return sg, z * sg, sg * (rho + torch.clamp(6.0 * e / U, max=3.0))


def ln_twin(x, gamma, beta, eps, K, z=None, rs=None, dy=None, dadd=None, *, eps_out=False, unbiased=False,
            second_order=False, saturated=False):
    """fp64 LayerNorm forward and backward in closed form, with the S of test_layernorm_against_fp64.  x (rows, C), z the
    gate or None, rs the per-ROW factor (rows,) or None, all fp64.  Every quantity of a row depends on that row alone
    (the column sums dgamma / dbeta apart), so a non-finite element poisons exactly what reads it."""
    C = x.shape[1]
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    var = (xc * xc).sum(-1, keepdim=True) / (C - 1 if unbiased else C)
    r = 1.0 / (var.sqrt() + eps) if eps_out else torch.rsqrt(var + eps)
    xh = xc * r
    b = beta if beta is not None else torch.zeros_like(gamma)
    n = xh * gamma + b
    rsr = rs[:, None] if rs is not None else torch.ones_like(mu)
    if z is not None:
        sg, s, ds = _sig_terms(z)
    else:
        sg, s, ds = None, torch.ones_like(x), None
    xha = xh.abs() + r * x.abs().mean(-1, keepdim=True)
    S_ln = gamma.abs() * xha + b.abs()
    out = dict(y=n * s * rsr, mean=mu[:, 0], rstd=r[:, 0], xh=xh, n=n, S_y=S_ln * s.abs() * rsr.abs(),
               S_mean=x.abs().mean(-1), S_rstd=r[:, 0].clone())
    if second_order:
        D = K["mean"] * U * x.abs().mean(-1)
        out["S_rstd"] = out["S_rstd"] + 0.5 * r[:, 0] ** 3 * D * D / (K["rstd"] * U)
    if saturated:
        f = (n * rsr * z).abs()
        out["S_y"] = out["S_y"] + f * ds / K["y"] + underflow_S(f.reshape(-1), K["y"]).view_as(f)
    if dy is None:
        return out
    gpre = dy * s * rsr
    t = gpre * gamma
    m1, m2 = t.mean(-1, keepdim=True), (t * xh).mean(-1, keepdim=True)
    dx = r * (t - m1 - xh * m2)
    gabs = gpre.abs()
    if saturated:                                          # the error of silu^ inside gpre, as a magnitude of its own
        f = (dy * rsr * z).abs()
        gabs = gabs + f * ds / K["dx"] + underflow_S(f.reshape(-1), K["dx"]).view_as(f)
    gg = gabs * gamma.abs()
    S_dx = r * (gg + gg.mean(-1, keepdim=True) + xha * (gg * xha).mean(-1, keepdim=True))
    if dadd is not None:
        dx, S_dx = dx + dadd, S_dx + dadd.abs()
    out.update(dx=dx, S_dx=S_dx, dgamma=(gpre * xh).sum(0), dbeta=gpre.sum(0), S_dg=(gabs * xha).sum(0), S_db=gabs.sum(0))
    if z is not None:
        a = dy * rsr
        out["dz"] = a * n * sg * (1.0 + z * (1.0 - sg))
        out["S_dz"] = a.abs() * sg * (1.0 + z.abs() * (1.0 - sg)) * S_ln
        if saturated:
            f = (a * n).abs() * (1.0 + z.abs())
            out["S_dz"] = out["S_dz"] + f * ds / K["dz"] + underflow_S(f.reshape(-1), K["dz"]).view_as(f)
    return out


def _sigmoid32(z):
    """sigmoid_f of csrc/layernorm.hip in fp32 torch ops: 1 / (1 + exp2(-z log2 e))"""
    return 1.0 / (1.0 + torch.exp2(-z * torch.tensor(LOG2E, dtype=torch.float32, device=z.device)))


def ln_emulate(x, gamma, beta, eps, z=None, rs=None, dy=None, dadd=None, *, onepass=False, eps_out=False):
    """the kernels' arithmetic in fp32 torch ops (torch's own summation order stands in for the lanes and DPP levels): two
    passes over the row, the variance around the computed mean, rsqrt(var + eps).  Wrong variants: ``onepass``
    (E[x^2] - E[x]^2) and ``eps_out`` (1 / (sqrt(var) + eps))."""
    f32 = torch.float32
    assert x.dtype == f32
    C = x.shape[1]
    inv = torch.tensor(1.0 / C, dtype=f32, device=x.device)
    mu = x.sum(-1, keepdim=True) * inv
    if onepass:
        var = (x * x).sum(-1, keepdim=True) * inv - mu * mu
    else:
        var = ((x - mu) * (x - mu)).sum(-1, keepdim=True) * inv
    r = 1.0 / (var.sqrt() + eps) if eps_out else torch.rsqrt(var + eps)
    b = beta if beta is not None else torch.zeros_like(gamma)
    y = (x - mu) * r * gamma + b
    rsr = rs[:, None] if rs is not None else None
    if z is not None:
        s0 = _sigmoid32(z)
        y = y * (z * s0)
    if rsr is not None:
        y = y * rsr
    out = dict(y=y, mean=mu[:, 0], rstd=r[:, 0])
    if dy is None:
        return out
    gv = dy * rsr if rsr is not None else dy
    xh = (x - mu) * r
    if z is not None:
        out["dz"] = gv * (xh * gamma + b) * s0 * (z * (1.0 - s0) + 1.0)
        gv = gv * (z * s0)
    t = gv * gamma
    m1, m2 = t.sum(-1, keepdim=True) * inv, (t * xh).sum(-1, keepdim=True) * inv
    dx = r * (t - m1 - xh * m2)
    if dadd is not None:
        dx = dx + dadd
    out.update(dx=dx, dgamma=(gv * xh).sum(0), dbeta=gv.sum(0))
    assert all(v.dtype == f32 for v in out.values())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# non-finite containment

POISONS = (NAN, INF, -INF)


def contained(got, ref, S, K):
    """(ratio over the entries where the twin is finite, share of those entries, ok): ok is False when the kernel is
    non-finite where the twin is finite, finite where the twin is not, or S is not finite where the twin is"""
    fin = torch.isfinite(ref)
    ok = bool(torch.isfinite(got[fin]).all()) and bool((~torch.isfinite(got[~fin])).all()) and bool(torch.isfinite(S[fin]).all())
    r = 0.0
    if ok and bool(fin.any()):
        r = float(((got[fin].double() - ref[fin]).abs() / (K * U * S[fin] + 1e-300)).max())
    return r, float(fin.double().mean()), ok


def ln_poison_rows(rows):
    """the first row, the last row, and the rows read by a final prefetch step: the last row that wave 0 walks, for every
    grid the host code can choose -- forward and backward launch min(ceil(rows / 4), 256 occ) workgroups of four waves with
    their own occupancy occ in 1 .. 8 (csrc/layernorm.hip fwd_grid, bwd_grid), the backward at most bwd_blocks (512 .. 2048,
    also a multiple of 256 or the 2 MB quotient).  Where every wave has one row, a middle row.  At most 10 rows."""
    blocks = -(-rows // 4)
    out = [0, rows - 1]
    for occ in range(1, 9):
        nwaves = 4 * min(blocks, 256 * occ)
        out.append(((rows - 1) // nwaves) * nwaves if rows > nwaves else rows // 2)
    return sorted(set(out))


def ln_last_row_of_wave0(rows, nwaves):
    return ((rows - 1) // nwaves) * nwaves if rows > nwaves else rows // 2


def up_adjoint(g):
    """fp64 adjoint of the bilinear x2 of (B, 2H, 2W, C) -> (B, H, W, C) as a gather: input index i collects the outputs
    2i - 1 .. 2i + 2 that exist, weights 1/4, 3/4, 3/4, 1/4, and at a border the weight an output loses to the clamp goes to
    the edge pixel (output 0 is x[0], output 2n - 1 is x[n - 1]).  A term is formed only where the output exists: the value
    autograd gives for finite g, without the 0 * g[0] that autograd of the clamped weights sends to x[1]."""
    def axis(t, dim):
        n2 = t.shape[dim]
        n = n2 // 2
        i = torch.arange(n, device=t.device)
        acc = None
        for k, w in enumerate((0.25, 0.75, 0.75, 0.25)):
            o = 2 * i - 1 + k
            ok = (o >= 0) & (o < n2)
            wk = torch.full((n,), w, dtype=torch.float64, device=t.device)
            # the clamp: output 0 reads x[0] with weight 1 (k = 1 at i = 0), output 2n - 1 reads x[n - 1] with weight 1
            wk = torch.where((o == 0) | (o == n2 - 1), torch.ones_like(wk), wk)
            shape = [1] * t.dim()
            shape[dim] = n
            term = t.index_select(dim, o.clamp(0, n2 - 1)) * wk.view(shape)
            term = torch.where(ok.view(shape), term, torch.zeros_like(term))
            acc = term if acc is None else acc + term
        return acc
    return axis(axis(g, 1), 2)


def up_readers(H, W, y, x):
    """the output pixels of the x2 forward that read input pixel (y, x) (a tap with weight 0 at the low border included: the
    index arithmetic is ATen's, where output 0 is 1 * x[0] + 0 * x[1]) and the input pixels of the adjoint that read OUTPUT
    pixel (y, x)"""
    def fwd_axis(n, i):
        out = set()
        for o in range(2 * n):
            src = max((o + 0.5) * 0.5 - 0.5, 0.0)
            i0 = int(src)
            if i in (i0, min(i0 + 1, n - 1)):
                out.add(o)
        return out

    def adj_axis(n, o):
        return {i for i in range(n) if 2 * i - 1 <= o <= 2 * i + 2}
    return ({(a, b) for a in fwd_axis(H, y) for b in fwd_axis(W, x)}, {(a, b) for a in adj_axis(H, y) for b in adj_axis(W, x)})


def scales_pow2(n, seed):
    """n scales 2^e, e drawn from -40 .. 40"""
    g = torch.Generator().manual_seed(seed)
    return 2.0 ** torch.randint(-40, 41, (n,), generator=g).float()


# ---------------------------------------------------------------------------------------------------------------------
# depthwise conv 3x3 + SiLU (csrc/dwconv.hip): the three smallest shapes of tests/test_dwconv_shapes_gpu.py that take the
# whole-plane kernel with one strip, with several, and the two-launch kernel above the 48 KiB line

DW_CASES = [(2, 3, 6, 8), (2, 4, 34, 64), (1, 2, 96, 61)]
DW_VALUES = [s * v for v in GATES for s in (1.0, -1.0)]


def dw_rounds(case):
    """runs of ``dw_saturated_inputs`` after which every value of DW_VALUES has been the pre-activation of a plane"""
    return -(-len(DW_VALUES) // (case[0] * case[1]))


def dw_saturated_inputs(case, rnd, seed, orders=2):
    """x (B, d, H, W), w (d, 1, 3, 3), b (d), g2 (B, orders, d, HW), fp32 on the CPU.  Plane (b, c) has the interior
    pre-activation v = DW_VALUES[(rnd B d + b d + c) mod 12] (+-0.1 %): positive weights, the bias of channel c half the
    value of its first plane, and an input of one sign per plane, (v - bias) / sum(w) (1 + 0.001 rand).  Towards the border
    fewer taps count and the pre-activation falls off towards the bias: the values in between are visited as well."""
    B, d, H, W = case
    g = torch.Generator().manual_seed(seed)
    w = 0.05 + 0.3 * torch.randn(d, 1, 3, 3, generator=g).abs()
    v = torch.tensor([[DW_VALUES[(rnd * B * d + b * d + c) % len(DW_VALUES)] for c in range(d)] for b in range(B)])
    bias = 0.5 * v[0]
    x = ((v - bias[None]) / w.sum((1, 2, 3))[None])[:, :, None, None] * (1.0 + 0.001 * torch.rand(B, d, H, W, generator=g))
    return x, w, bias, torch.randn(B, orders, d, H * W, generator=g), v


def dw_inputs(case, seed, orders=2):
    """the N(0, 1) inputs of tests/test_dwconv_shapes_gpu.py, on the CPU"""
    B, d, H, W = case
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, d, H, W, generator=g), 0.3 * torch.randn(d, 1, 3, 3, generator=g), 0.1 * torch.randn(d, generator=g),
            torch.randn(B, orders, d, H * W, generator=g))


def dw_K(case, plane):
    """test_dwconv_silu_against_fp64: out2 16, dx 33, the sums (a workgroup's serial depth) + 24 + the atomics or slots;
    gpre 24 (tests/test_dwconv_shapes_gpu.py)"""
    B, d, H, W = case
    tiles = 1 if plane else -(-H // 32) * -(-W // 32)
    Kr = (-(-H * W // 256) if plane else 4) + 6 + 3 + 24 + B * tiles
    return dict(out2=16, gpre=24, dx=33, dweight=Kr, dbias=Kr)


def _dw_parts(x, w, b, g2, orders, dref):
    """pre-activation, its magnitude, the summed upstream gradient and its magnitude, the padded input"""
    import torch.nn.functional as F
    B, d, H, W = x.shape
    pre, ab = dref(x, w, b)
    gs = lambda t: t[:, 0].view(B, d, H, W) + (t[:, 1].view(B, d, W, H).transpose(2, 3) if orders == 2 else 0.0)
    return pre, ab + b.abs().view(1, d, 1, 1), gs(g2), gs(g2.abs()), F.pad(x, (1, 1, 1, 1))


def _dw_sums(gpre, xpad, H, W):
    return (torch.stack([(gpre * xpad[:, :, i:i + H, j:j + W]).sum((0, 2, 3)) for i in range(3) for j in range(3)], 1), gpre.sum((0, 2, 3)))


def dw_twin(x, w, b, g2, orders, K, saturated=False, clamp=None):
    """fp64 forward and backward with the S of test_dwconv_silu_against_fp64, every stencil as nine shifted adds (a
    non-finite pixel reaches its 3 x 3 neighbours and nothing else).  ``saturated`` adds the argument-error and underflow
    terms of the module docstring to S_out2 and S_gpre (and through S_gpre to dx, dweight, dbias).  ``clamp``: the wrong
    variant whose pre-activation is clamped to +-clamp."""
    B, d, H, W = x.shape
    pre, S_pre, gsum, gabs, xpad = _dw_parts(x, w, b, g2, orders, _dw_ref)
    if clamp is not None:
        pre = pre.clamp(-clamp, clamp)
    sg, y, ds = _sig_terms(pre)
    S_y = S_pre * (1.1 + pre.abs())
    gpre = gsum * sg * (1.0 + pre * (1.0 - sg))
    S_gpre = gabs * (1.1 + S_pre)
    if saturated:
        f = pre.abs()
        S_y = S_y + f * ds / K["out2"] + underflow_S(f.reshape(-1), K["out2"]).view_as(f)
        f = gabs * (1.0 + pre.abs())
        S_gpre = S_gpre + f * ds / K["gpre"] + underflow_S(f.reshape(-1), K["gpre"]).view_as(f)
    wf = w.flip(2, 3)
    dw, db = _dw_sums(gpre, xpad, H, W)
    S_dw, S_db = _dw_sums(S_gpre, xpad.abs(), H, W)
    return dict(out2=_two_orders(y, orders), S_out2=_two_orders(S_y, orders), gpre=gpre, S_gpre=S_gpre, dx=_dw_ref(gpre, wf, None)[0],
                S_dx=_dw_ref(S_gpre, wf.abs(), None)[0], dweight=dw, S_dweight=S_dw, dbias=db, S_dbias=S_db, pre=pre)


def dw_emulate(x, w, b, g2, orders):
    """the kernels' arithmetic in fp32 torch ops: nine products and adds, sigmoid as rcp(1 + exp2(-p log2 e)), silu' as
    s (p (1 - s) + 1), the transposed stencil and the sums in torch's order"""
    assert x.dtype == torch.float32
    B, d, H, W = x.shape
    pre, _, gsum, _, xpad = _dw_parts(x, w, b, g2, orders, _dw_ref)
    s0 = _sigmoid32(pre)
    gpre = gsum * (s0 * (pre * (1.0 - s0) + 1.0))
    dw, db = _dw_sums(gpre, xpad, H, W)
    out = dict(out2=_two_orders(pre * s0, orders), gpre=gpre, dx=_dw_ref(gpre, w.flip(2, 3), None)[0], dweight=dw, dbias=db)
    assert all(v.dtype == torch.float32 for v in out.values())
    return out


def dw_neighbours(H, W, h, w_, reach=1):
    """the pixels within ``reach`` of (h, w_) inside the plane"""
    return {(a, b) for a in range(max(0, h - reach), min(H, h + reach + 1)) for b in range(max(0, w_ - reach), min(W, w_ + reach + 1))}


# ---------------------------------------------------------------------------------------------------------------------
# twins and poison plans of the plane ops, colscale, merge and pair-sum (device-agnostic; the CPU test takes the finite
# share from them, the GPU test holds the kernels to them)

def plane_twin(x, g, s, dm, dmx):
    """fp64 of the four plane ops with the S of test_plane_ops_against_fp64; the maximum and its count as torch.amax and ==
    give them (a NaN is the maximum of its plane and equals nothing)"""
    P, hw = x.shape
    xd, gd, sd = x.double(), g.double(), s.double()[:, None]
    mx = xd.amax(1)
    hit = xd == mx[:, None]
    cnt = hit.sum(1).double()
    share = torch.where(hit, (dmx.double() / cnt)[:, None].expand(P, hw), torch.zeros_like(xd))
    share_abs = torch.where(hit, (dmx.double().abs() / cnt)[:, None].expand(P, hw), torch.zeros_like(xd))
    return dict(mean=xd.mean(1), S_mean=xd.abs().mean(1), max=mx, count=cnt, scale=xd * sd, S_scale=(xd * sd).abs(),
                dot=(gd * xd).sum(1), S_dot=(gd * xd).abs().sum(1), gate_bwd=gd * sd + dm.double()[:, None] / hw + share,
                S_gate_bwd=(gd * sd).abs() + dm.double().abs()[:, None] / hw + share_abs)


PLANE_POISON_P = 24                     # one poisoned plane of x and one of g among 24: 22 / 24 of every output stay finite


def plane_poison_inputs(hw, value, seed, device="cpu"):
    """24 tied planes; one pixel of plane 5 of x and one pixel of plane 17 of g (the dy of dot and gate_bwd) hold ``value``"""
    P = PLANE_POISON_P
    gen = torch.Generator().manual_seed(seed)
    x = plane_inputs(P, hw, ("tied",), seed)
    g, s, dm, dmx = torch.randn(P, hw, generator=gen), torch.randn(P, generator=gen), torch.randn(P, generator=gen), torch.randn(P, generator=gen)
    x[5, hw // 2] = value
    g[17, hw - 1] = value
    return tuple(t.to(device) for t in (x, g, s, dm, dmx))


def merge_ref(p4, nh, swapped=False):
    """fp64 merge of (B, 4, d, L) planes, its S, and the split of (B, H, W, d); ``swapped``: the memory orders exchanged"""
    B, _, d, L = p4.shape
    _, H, W, _ = nh.shape
    q = p4.double()
    row = lambda t: t.view(B, d, H, W).permute(0, 2, 3, 1)
    col = lambda t: t.view(B, d, W, H).permute(0, 3, 2, 1)
    terms = [col(q[:, 0]), col(q[:, 1]), row(q[:, 2]), row(q[:, 3])] if swapped else [row(q[:, 0]), row(q[:, 1]), col(q[:, 2]), col(q[:, 3])]
    n = nh.permute(0, 3, 1, 2)
    return sum(terms), sum(t.abs() for t in terms), torch.stack([n.reshape(B, d, L), n.transpose(2, 3).reshape(B, d, L)], 1)


MERGE_POISON = ((2, 33, 15, 17), (1, 2, 32, 100), (1, 14, 16, 32))       # shape, the element of planes4, the element of nhwc
PAIR_POISON = ((2, 4100, 0), (20, 5, 1))                                 # (n_outer, inner, offset): src[1, 1, -1] and acc[0, 0]
CS_POISON_ROWS = 300                                                     # dy[rows - 1, 7] and x[0, C - 1]


def colscale_poison_inputs(C, value, seed, device="cpu"):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(CS_POISON_ROWS, C, generator=gen).abs() + 0.01
    dy = 0.5 * x + torch.randn(CS_POISON_ROWS, C, generator=gen)
    s = torch.randn(C, generator=gen)
    dy[CS_POISON_ROWS - 1, 7], x[0, C - 1] = value, value
    return tuple(t.to(device) for t in (dy, x, s))


def pair_poison_inputs(no, inner, value, seed, device="cpu"):
    gen = torch.Generator().manual_seed(seed)
    src, acc = torch.randn(no, 2, inner, generator=gen), torch.randn(no, inner, generator=gen)
    src[1, 1, inner - 1], acc[0, 0] = value, value
    return src.to(device), acc.to(device)


def flushed(z, values, below=-15.0):
    """the wrong variant whose sigmoid is flushed to zero below ``below``: ``values`` with zeros wherever z < below"""
    return torch.where(z < below, torch.zeros_like(values), values)
