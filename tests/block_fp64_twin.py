"""Plain-torch twins of the five blocks of the model, written from the formulas; the reference for the layer that
stitches kernels into blocks (anchored and exercised in tests/test_blocks_fp64_cpu.py).  Nothing of
sigma_amd is imported here.

Each twin takes the block's ``state_dict`` (names as in the model), its inputs and -- for training mode -- the
per-sample stochastic-depth factors (mask / keep probability, one value per sample) as explicit arguments, and works in
the dtype and on the device of what it is given.  ``run`` wraps a twin into forward + backward and returns every output,
input gradient and parameter gradient by name.

    VSSBlock          out = x + f * out_proj( LN_out(SS2D(silu(dwconv(xi)))) * silu(z) ),   [xi | z] = in_proj(LN(x))
    CVSSDecoderBlock  t = x * scale1 + f * SS2D-branch(LN1(x));  out = t * scale2 + CAB(LN2(t))
                      CAB = conv3x3 (C -> C/3), GELU, conv3x3 (C/3 -> C), times sigmoid(fc(avg) + fc(max))
    CrossMamba        two 1-D scans over the row-major tokens; each modality's scan reads the C of the OTHER modality
    ConcatMamba       one sequence [rgb tokens ; x tokens] scanned forwards and backwards, the two results added;
                      each half gated by the pooled in_proj output of the other modality, concatenated, out_proj
    PatchMerging2D    pad to even sizes, gather the 2 x 2 neighbours into 4C channels (block = 2 * w parity + h parity),
                      LN(4C), Linear(4C -> out)

SS2D: the four sequences of an image are k = 0 row-major, 1 column-major, 2 reversed row-major, 3 reversed
column-major.  Per direction [dt | B | C] = x_proj_weight[k] @ seq, delta = dt_projs_weight[k] @ dt, then the selective
scan  h_t = exp(softplus(delta_t + bias) A) h_{t-1} + softplus(.) B_t u_t,  y_t = C_t . h_t + D u_t  with A = -exp(A_logs);
the four results are put back into row-major order and added.

Every matrix product goes through ``mm``.  Inside ``noise(seed)`` it returns the product plus
sigma * rms(product) * randn, and the gradient it hands to each operand plus sigma * rms(gradient) * randn, sigma = 2e-5:
what a block computes when every GEMM is as wrong as tests/test_gemm_gpu.py::_assert_close lets a two-piece GEMM be.

``wrong`` names a plausible defect of the layer that stitches kernels together (the negative controls; only this file's
code runs in them), see WRONG.
"""
from __future__ import annotations

import contextlib
import math

import torch

SIGMA = 2e-5          # relative rms error the project asserts for its two-piece GEMMs (tests/test_gemm_gpu.py::_assert_close)
U23 = 2.0 ** -23

# defect -> (block kind, the slice that must leave the bound)
WRONG = {
    "dt_weight_perm": ("vss", "op.dt_projs_weight"),       # d dt_projs_weight left in the kernels' group order [0, 2, 1, 3]
    "dA_no_A": ("vss", "op.A_logs"),                       # d A_logs = dA instead of dA * A
    "du_rev_dropped": ("vss", "dx0"),                      # du of the two reversed directions missing from d x
    "residual_grad": ("vss", "dx0"),                       # the residual's gradient not joined to the LayerNorm backward
    "mask_unscaled": ("vss", "out0"),                      # stochastic depth: mask not divided by the keep probability
    "pair_one_direction": ("conmb", "op.x_proj_weight"),   # the summed pair hands its gradient to the forward direction only
    "c_not_swapped": ("cromb", "out0"),                    # each modality scanned with its own C
    "scale1_operand": ("cvss", "scale1"),                  # d scale1 from the branch instead of the block input
    "merge_order": ("merge", "out0"),                      # channel blocks in (h parity, w parity) order
}

_NOISE = {"seed": None, "sigma": 0.0, "gens": {}}


@contextlib.contextmanager
def noise(seed: int, sigma: float = SIGMA):
    """every ``mm`` inside the block is perturbed; the draws depend on ``seed`` (and the generator of the device the
    tensors live on, made at the first draw) alone"""
    old = dict(_NOISE)
    _NOISE.update(seed=int(seed), sigma=float(sigma), gens={})
    try:
        yield
    finally:
        _NOISE.update(old)


def _perturbed(t):
    if t is None or t.numel() == 0:
        return t
    gen = _NOISE["gens"].get(t.device)
    if gen is None:
        gen = _NOISE["gens"][t.device] = torch.Generator(device=t.device).manual_seed(_NOISE["seed"])
    z = torch.randn(t.shape, generator=gen, device=t.device, dtype=t.dtype)
    return t + _NOISE["sigma"] * t.detach().pow(2).mean().sqrt() * z


class _NoisyOut(torch.autograd.Function):
    """forward: the product with its noise; backward: the gradient unchanged"""

    @staticmethod
    def forward(ctx, t):
        return _perturbed(t)

    @staticmethod
    def backward(ctx, g):
        return g


class _NoisyGrad(torch.autograd.Function):
    """forward: the operand unchanged; backward: its gradient with noise"""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return _perturbed(g)


def mm(a, b):
    """a @ b (torch.matmul broadcasting): the one door every matrix product of the twins goes through"""
    if _NOISE["seed"] is None:
        return torch.matmul(a, b)
    return _NoisyOut.apply(torch.matmul(_NoisyGrad.apply(a), _NoisyGrad.apply(b)))


# ---------------------------------------------------------------------------------------------------------------------
# pieces

def linear(x, w, b=None):
    y = mm(x, w.transpose(0, 1))
    return y if b is None else y + b


def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def silu(x):
    return x * torch.sigmoid(x)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _shifted(x):
    """the nine zero-padded 3 x 3 neighbours of every pixel: (B, C, H, W) -> (B, C, 9, H, W), index 3 * ky + kx"""
    B, C, H, W = x.shape
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    return torch.stack([xp[:, :, i:i + H, j:j + W] for i in range(3) for j in range(3)], dim=2)


def dwconv3x3(x, w, b):
    """depthwise: w (C, 1, 3, 3)"""
    return (_shifted(x) * w.reshape(1, -1, 9, 1, 1)).sum(2) + b.reshape(1, -1, 1, 1)


def conv3x3(x, w, b):
    """dense: w (Co, Ci, 3, 3), as a matrix product over the gathered neighbours"""
    B, C, H, W = x.shape
    cols = _shifted(x).reshape(B, C * 9, H * W)
    return (mm(w.reshape(w.shape[0], C * 9), cols) + b.reshape(1, -1, 1)).reshape(B, -1, H, W)


def recurrence(a, w):
    """h_t = a_t h_{t-1} + w_t along the last dimension (h_{-1} = 0), by doubling: after the step of distance d, (a_t, w_t)
    composes the positions t - 2d + 1 .. t.  Out of place, so autograd differentiates it."""
    L = a.shape[-1]
    d = 1
    while d < L:
        w = torch.cat([w[..., :d], w[..., d:] + a[..., d:] * w[..., :-d]], dim=-1)
        if 2 * d < L:
            a = torch.cat([a[..., :d], a[..., d:] * a[..., :-d]], dim=-1)
        d *= 2
    return w


def selective_scan(u, delta, A, Bm, Cm, D, bias):
    """u, delta (B, G * rows, L); A (G * rows, N); Bm, Cm (B, G, N, L); D, bias (G * rows) -> y (B, G * rows, L)"""
    Bsz, KD, L = u.shape
    G, N = Bm.shape[1], Bm.shape[2]
    rows = KD // G
    dl = torch.nn.functional.softplus(delta + bias[None, :, None], threshold=20.0)
    a = torch.exp(dl.unsqueeze(2) * A[None, :, :, None])                           # (B, KD, N, L)
    Bx = Bm.unsqueeze(2).expand(Bsz, G, rows, N, L).reshape(Bsz, KD, N, L)
    Cx = Cm.unsqueeze(2).expand(Bsz, G, rows, N, L).reshape(Bsz, KD, N, L)
    h = recurrence(a, (dl * u).unsqueeze(2) * Bx)
    return (h * Cx).sum(2) + D[None, :, None] * u


class _NegExpNoA(torch.autograd.Function):
    """-exp(A_logs) whose backward forgets the factor A"""

    @staticmethod
    def forward(ctx, a_logs):
        return -torch.exp(a_logs)

    @staticmethod
    def backward(ctx, g):
        return g


class _GradPerm(torch.autograd.Function):
    """identity whose gradient comes back with entries 1 and 2 of the first dimension exchanged"""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g[[0, 2, 1, 3]]


class _ScaleWrongOperand(torch.autograd.Function):
    """x * s whose d s is taken from ``other``"""

    @staticmethod
    def forward(ctx, x, s, other):
        ctx.save_for_backward(s, other)
        return x * s

    @staticmethod
    def backward(ctx, g):
        s, other = ctx.saved_tensors
        return g * s, (g * other).reshape(-1, s.numel()).sum(0), None


def ss2d_core(x, p, pre, wrong=None):
    """x (B, d, H, W) -> (B, H, W, d): the four-direction scan and its merge, parameters p[pre + ...]"""
    B, d, H, W = x.shape
    L = H * W
    xw, dtw, dtb = p[pre + "x_proj_weight"], p[pre + "dt_projs_weight"], p[pre + "dt_projs_bias"]
    a_logs, Ds = p[pre + "A_logs"], p[pre + "Ds"]
    R, N = dtw.shape[2], a_logs.shape[1]
    if wrong == "dt_weight_perm":
        dtw = _GradPerm.apply(dtw)
    rm = x.reshape(B, d, L)
    cm = x.transpose(2, 3).reshape(B, d, L)
    xs = torch.stack([rm, cm, rm.flip(-1), cm.flip(-1)], dim=1)                    # (B, 4, d, L)
    proj = mm(xw.unsqueeze(0), xs)                                                 # (B, 4, R + 2N, L)
    dt, Bm, Cm = proj[:, :, :R], proj[:, :, R:R + N], proj[:, :, R + N:]
    delta = mm(dtw.unsqueeze(0), dt)                                               # (B, 4, d, L)
    A = _NegExpNoA.apply(a_logs) if wrong == "dA_no_A" else -torch.exp(a_logs)
    us = xs
    if wrong == "du_rev_dropped":
        us = torch.stack([rm, cm, rm.flip(-1).detach(), cm.flip(-1).detach()], dim=1)
    ys = selective_scan(us.reshape(B, 4 * d, L), delta.reshape(B, 4 * d, L), A, Bm, Cm, Ds, dtb.reshape(-1)).reshape(B, 4, d, L)
    y_rm = ys[:, 0] + ys[:, 2].flip(-1)
    y_cm = ys[:, 1] + ys[:, 3].flip(-1)
    y = y_rm + y_cm.reshape(B, d, W, H).transpose(2, 3).reshape(B, d, L)
    return y.transpose(1, 2).reshape(B, H, W, d)


def ss2d(x, p, pre, wrong=None):
    """the SS2D operator on a normalised (B, H, W, C) input -> (B, H, W, C)"""
    xz = linear(x, p[pre + "in_proj.weight"])
    d = xz.shape[-1] // 2
    xi, z = xz[..., :d], xz[..., d:]
    xi = silu(dwconv3x3(xi.permute(0, 3, 1, 2), p[pre + "conv2d.weight"], p[pre + "conv2d.bias"]))
    y = ss2d_core(xi, p, pre, wrong)
    y = layer_norm(y, p[pre + "out_norm.weight"], p[pre + "out_norm.bias"]) * silu(z)
    return linear(y, p[pre + "out_proj.weight"])


def _factor(f, like, wrong=None):
    """per-sample factors (B,) -> (B, 1, 1, 1), or 1 in eval mode"""
    if f is None:
        return 1.0
    f = f.to(like.dtype).to(like.device)
    if wrong == "mask_unscaled":
        f = (f != 0).to(like.dtype)
    return f.reshape(-1, 1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------
# blocks: (p, inputs, factors, wrong) -> tuple of outputs

def vss_block(p, inputs, factors=(None,), wrong=None):
    (x,) = inputs
    branch = ss2d(layer_norm(x, p["norm.weight"], p["norm.bias"]), p, "op.", wrong) * _factor(factors[0], x, wrong)
    return ((x.detach() if wrong == "residual_grad" else x) + branch,)


def cvss_block(p, inputs, factors=(None,), wrong=None):
    (x,) = inputs
    branch = ss2d(layer_norm(x, p["norm1.weight"], p["norm1.bias"]), p, "op.", wrong) * _factor(factors[0], x, wrong)
    if wrong == "scale1_operand":
        t = _ScaleWrongOperand.apply(x, p["scale1"], branch.detach()) + branch
    else:
        t = x * p["scale1"] + branch
    c = layer_norm(t, p["norm2.weight"], p["norm2.bias"]).permute(0, 3, 1, 2)
    c = conv3x3(c, p["conv_blk.cab.0.weight"], p["conv_blk.cab.0.bias"])
    c = conv3x3(gelu(c), p["conv_blk.cab.2.weight"], p["conv_blk.cab.2.bias"])
    w1, w2 = p["conv_blk.cab.3.fc.0.weight"].flatten(1), p["conv_blk.cab.3.fc.2.weight"].flatten(1)   # (C/30, C), (C, C/30)
    fc = lambda v: linear(silu(linear(v, w1)), w2)                                 # (B, C) -> (B, C)
    gate = torch.sigmoid(fc(c.mean(dim=(2, 3))) + fc(c.amax(dim=(2, 3))))
    c = c * gate[:, :, None, None]
    return (t * p["scale2"] + c.permute(0, 2, 3, 1),)


def cromb_block(p, inputs, factors=(None, None), wrong=None):
    x_rgb, x_e = inputs
    B, H, W, _ = x_rgb.shape
    conv = lambda t: silu(dwconv3x3(t.permute(0, 3, 1, 2), p["op.conv2d.weight"], p["op.conv2d.bias"])).flatten(2)
    s_rgb = conv(linear(x_rgb, p["op.in_proj.weight"]))                            # (B, d, L), one shared convolution
    s_e = conv(linear(x_e, p["op.in_proj_modalx.weight"]))
    N = p["op.CMA_ssm.A_log_1"].shape[1]

    def project(seq, i):
        dbl = mm(p[f"op.CMA_ssm.x_proj_{i}.weight"].unsqueeze(0), seq)            # (B, R + 2N, L)
        R = dbl.shape[1] - 2 * N
        return mm(p[f"op.CMA_ssm.dt_proj_{i}.weight"].unsqueeze(0), dbl[:, :R]), dbl[:, None, R:R + N], dbl[:, None, R + N:]

    dt1, B1, C1 = project(s_rgb, 1)
    dt2, B2, C2 = project(s_e, 2)
    if wrong == "c_not_swapped":
        C1, C2 = C2, C1
    y1 = selective_scan(s_rgb, dt1, -torch.exp(p["op.CMA_ssm.A_log_1"]), B1, C2, p["op.CMA_ssm.D_1"], p["op.CMA_ssm.dt_proj_1.bias"])
    y2 = selective_scan(s_e, dt2, -torch.exp(p["op.CMA_ssm.A_log_2"]), B2, C1, p["op.CMA_ssm.D_2"], p["op.CMA_ssm.dt_proj_2.bias"])
    y1 = layer_norm(y1.transpose(1, 2), p["op.CMA_ssm.out_norm_1.weight"], p["op.CMA_ssm.out_norm_1.bias"]).reshape(B, H, W, -1)
    y2 = layer_norm(y2.transpose(1, 2), p["op.CMA_ssm.out_norm_2.weight"], p["op.CMA_ssm.out_norm_2.bias"]).reshape(B, H, W, -1)
    o1 = linear(y1, p["op.out_proj_rgb.weight"])
    o2 = linear(y2, p["op.out_proj_e.weight"])
    return x_rgb + o1 * _factor(factors[0], o1, wrong), x_e + o2 * _factor(factors[1], o2, wrong)


def conmb_block(p, inputs, factors=(None,), wrong=None):
    x_rgb, x_e = inputs
    B, H, W, _ = x_rgb.shape
    HW = H * W
    p_rgb = linear(x_rgb, p["op.in_proj.weight"]).permute(0, 3, 1, 2)             # (B, d, H, W)
    p_e = linear(x_e, p["op.in_proj_modalx.weight"]).permute(0, 3, 1, 2)
    c_rgb = silu(dwconv3x3(p_rgb, p["op.conv2d.weight"], p["op.conv2d.bias"]))
    c_e = silu(dwconv3x3(p_e, p["op.conv2d_modalx.weight"], p["op.conv2d_modalx.bias"]))
    d = c_rgb.shape[1]
    seq = torch.cat([c_rgb.flatten(2), c_e.flatten(2)], dim=2)                     # (B, d, 2HW): rgb tokens first
    xs = torch.stack([seq, seq.flip(-1)], dim=1)                                   # (B, 2, d, L)
    dtw, a_logs = p["op.dt_projs_weight"], p["op.A_logs"]
    R, N = dtw.shape[2], a_logs.shape[1]
    proj = mm(p["op.x_proj_weight"].unsqueeze(0), xs)
    delta = mm(dtw.unsqueeze(0), proj[:, :, :R])
    ys = selective_scan(xs.reshape(B, 2 * d, -1), delta.reshape(B, 2 * d, -1), -torch.exp(a_logs), proj[:, :, R:R + N],
                        proj[:, :, R + N:], p["op.Ds"], p["op.dt_projs_bias"].reshape(-1)).reshape(B, 2, d, -1)
    back = ys[:, 1].flip(-1)
    y = ys[:, 0] + (back.detach() if wrong == "pair_one_direction" else back)
    y_rgb = layer_norm(y[..., :HW].transpose(1, 2), p["op.out_norm1.weight"], p["op.out_norm1.bias"]).reshape(B, H, W, d)
    y_e = layer_norm(y[..., HW:].transpose(1, 2), p["op.out_norm2.weight"], p["op.out_norm2.bias"]).reshape(B, H, W, d)
    gate = lambda v, n: torch.sigmoid(linear(silu(linear(v, p[f"op.{n}.0.weight"])), p[f"op.{n}.2.weight"]))
    g_rgb = gate(p_rgb.mean(dim=(2, 3)), "fc1")                                    # each modality gated by the OTHER one's pool
    g_e = gate(p_e.mean(dim=(2, 3)), "fc2")
    cat = torch.cat([y_rgb * g_e[:, None, None, :], y_e * g_rgb[:, None, None, :]], dim=-1)
    o = linear(cat, p["op.out_proj.weight"])
    return (x_rgb + x_e + o * _factor(factors[0], o, wrong),)


def merge_block(p, inputs, factors=(), wrong=None):
    (x,) = inputs
    B, H, W, C = x.shape
    x = torch.nn.functional.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    ev, od = slice(0, None, 2), slice(1, None, 2)
    parts = [x[:, ev, ev], x[:, od, ev], x[:, ev, od], x[:, od, od]]               # [h parity][w parity]: block 2 * wp + hp
    if wrong == "merge_order":
        parts = [parts[0], parts[2], parts[1], parts[3]]
    x = torch.cat(parts, dim=-1)
    return (linear(layer_norm(x, p["norm.weight"], p["norm.bias"]), p["reduction.weight"]),)


BLOCKS = {"vss": vss_block, "cvss": cvss_block, "cromb": cromb_block, "conmb": conmb_block, "merge": merge_block}


# ---------------------------------------------------------------------------------------------------------------------
# forward + backward, slices, metric

def run(kind, sd, inputs, gys, factors=None, dtype=torch.float64, device=None, noise_seed=None, wrong=None):
    """forward + backward of twin ``kind``: {"out<i>", "dx<i>", <parameter name>: gradient} in ``dtype``"""
    device = device if device is not None else inputs[0].device
    cast = lambda t: t.detach().to(device=device, dtype=dtype)
    p = {k: cast(v).requires_grad_() for k, v in sd.items()}
    xs = [cast(x).requires_grad_() for x in inputs]
    fn = BLOCKS[kind]
    kw = {} if factors is None else {"factors": tuple(factors)}
    ctx = noise(noise_seed) if noise_seed is not None else contextlib.nullcontext()
    with ctx:
        outs = fn(p, xs, wrong=wrong, **kw)
        leaves = xs + list(p.values())
        grads = torch.autograd.grad(outs, leaves, [cast(g) for g in gys], allow_unused=True)
    res = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    for i in range(len(xs)):
        res[f"dx{i}"] = grads[i]
    for k, g in zip(p, grads[len(xs):]):
        res[k] = g if g is not None else torch.zeros_like(p[k])
    return res


_STACKED = ("x_proj_weight", "dt_projs_weight", "dt_projs_bias", "A_logs", "Ds")


def slices(kind, name, t):
    """[(label, tensor)]: outputs and input gradients per sample, the stacked SSM parameters per direction, the two
    halves of an SS2D in_proj, every other parameter whole"""
    leaf = name.split(".")[-1]
    if name.startswith(("out", "dx")) and name[-1].isdigit() and "." not in name:
        return [(f"{name}[b={b}]", t[b]) for b in range(t.shape[0])]
    if leaf in _STACKED:
        K = 2 if kind == "conmb" else 4
        return [(f"{name}[k={k}]", s) for k, s in enumerate(t.reshape(K, -1))]
    if kind in ("vss", "cvss") and name == "op.in_proj.weight":
        h = t.shape[0] // 2
        return [(f"{name}[x]", t[:h]), (f"{name}[z]", t[h:])]
    return [(name, t)]


def slice_errors(kind, got, ref):
    """{label: ||got - ref|| / ||ref||} over every slice of every tensor of ``ref``; a slice whose reference is exactly
    zero gives 0 if ``got`` is exactly zero there and inf otherwise"""
    out = {}
    for name, r in ref.items():
        g = got[name].detach().to(device=r.device, dtype=torch.float64)
        assert g.shape == r.shape, (name, tuple(g.shape), tuple(r.shape))
        for (label, gs), (_, rs) in zip(slices(kind, name, g), slices(kind, name, r.to(torch.float64))):
            den = float(rs.norm())
            num = float((gs - rs).norm())
            if not math.isfinite(num):
                out[label] = math.inf
            elif den == 0.0:
                out[label] = 0.0 if num == 0.0 else math.inf
            else:
                out[label] = num / den
    return out


def twin_reference(kind, sd, inputs, gys, factors=None, device=None, seeds=(1, 2, 3)):
    """(ref64, e32, e_pert): the clean float64 twin, and per slice the float32 twin's and the noisy float64 twin's
    (largest of three seeds) distance from it"""
    ref = run(kind, sd, inputs, gys, factors, torch.float64, device)
    e32 = slice_errors(kind, run(kind, sd, inputs, gys, factors, torch.float32, device), ref)
    e_pert = {k: 0.0 for k in e32}
    for s in seeds:
        e = slice_errors(kind, run(kind, sd, inputs, gys, factors, torch.float64, device, noise_seed=s), ref)
        e_pert = {k: max(v, e[k]) for k, v in e_pert.items()}
    return ref, e32, e_pert


def bound(e32, e_pert):
    """bound(slice) = 2 (e32 + e_pert) + 2^-23"""
    return {k: 2.0 * (e32[k] + e_pert[k]) + U23 for k in e32}
