"""Inputs, error bounds and an fp32 emulation of the fused upsample + cross-entropy kernels (csrc/deepsup.hip), shared by
tests/test_deepsup_gpu.py (the kernels against the fp64 twin) and tests/test_deepsup_cpu.py (the emulation against the same
bounds on the same inputs, and the wrong variants of the twin against them, so that the GPU test cannot pass vacuously).
No GPU is needed to import or run anything here.

Inputs (``deepsup_inputs``): N(0, 3^2) coarse logits with NaN behind the classes, labels with ~10 % ignore_index, one
negative label and (where the pitch leaves a pad) one label inside the pad, from a CPU generator.

Bounds, |got - ref| <= u (...) with u = 2^-24; exp / log within 2 ulp as for the plain kernels.  Notation for a fine pixel P:
z = the exact interpolated row of the fp32 coarse logits, l = lse(z), p = softmax(z), A_c = the interpolation of |v_c| with
the same weights, Amax = max_c A_c.

z^        an interpolated logit is R_k = fma(ly, v_1k, (1 - ly) v_0k), z^ = fma(lx, R_1, (1 - lx) R_0): no v passes more
          than four roundings (the weights are exact for s a power of two), so |z^_c - z_c| <= 4 u A_c.
lse       the code of the plain kernels on the row z^: (C + 8) u (|l| + 1) (tests/test_loss_options_gpu.py); lse is
          1-Lipschitz in the max norm, so moving the row from z to z^ adds 4 u Amax:
              E_lse = u [(C + 8) (|l| + 1) + 4 Amax]
row loss  l^ - z^_y, one more rounding:  E_row = E_lse + u (4 A_y + |l - z_y|)
partial   [:, 0]: the rows of a workgroup are added by a thread (ceil(rows / (256 x 1024)) adds), across the wave (6) and
          across the four waves (4):  sum of the rows' E_row + (ceil(rows / 2^18) + 10) u sum of the rows' |row|.
          [:, 1]: whole numbers below 2^24, exact.
loss      the 1024 pairs are added by torch (a tree of depth <= 13), then one division:
              E_loss = (sum of E_partial + 13 u sum |partial[:, 0]|) / count + u |loss|
dlogits   an element is g sum_P wgt_P e_P, e_P = p^_c - [c == y], over up to N = (2 s)^2 fine pixels.
          p^_c = exp(z^_c - l^) carries the plain kernels' (C + 11) u (|z_c| + |l| + 1) p_c, and the interpolation moves
          z^_c by 4 u A_c and l^ by 4 u Amax:
              E_p = u p_c [(C + 11) (|z_c| + |l| + 1) + 4 A_c + 4 Amax]
          The subtraction and the product with g round once each (wgt = wy wx and its product inside the fma are exact /
          unrounded for s a power of two): 2 u |term|.  The summation in any order: N u sum |terms|.  With T = sum_P wgt_P |e_P|:
              E_dl = |g| [ sum_P wgt_P E_p(P) + (N + 2) u T ] + N 2^-126
          (the last term: the underflow threshold of fp32, for a product that is flushed).
Through the front end g = upstream / count is formed on the device: one more rounding, u |dl|.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.deepsup_fp64_twin import adjoint, interp_matrix, taps, twin, upsample

IGNORE = 255
U = 2.0 ** -24
SIGMA_CE_BLOCKS = 1024
# (B, h, w, s, nc, ld): the smallest shapes at which the kernels can go wrong
CASES = [(1, 1, 1, 4, 9, 12),        # every tap clamped
         (2, 2, 3, 16, 40, 40),      # every footprint clipped, batch stride
         (1, 3, 5, 8, 5, 8),         # an interior pixel, pitch above 4 ceil(nc / 4)
         (2, 5, 4, 4, 37, 40),
         (1, 4, 6, 16, 64, 64),      # register limit
         (1, 3, 3, 2, 1, 4),         # one class
         (1, 4, 4, 1, 9, 12),        # scale 1 is the plain loss
         (1, 2, 2, 32, 9, 12)]       # largest scale
CASE_IDS = ["%dx%dx%d_x%d_%d@%d" % c for c in CASES]


def deepsup_inputs(case, seed=0):
    """CPU tensors: buf (B, h, w, ld) fp32 with NaN in the pad, lab (B, h s, w s) int64"""
    B, h, w, s, nc, ld = case
    g = torch.Generator().manual_seed(1000 + seed)
    buf = torch.full((B, h, w, ld), float("nan"))
    buf[..., :nc] = torch.randn(B, h, w, nc, generator=g) * 3.0
    lab = torch.randint(0, nc, (B, h * s, w * s), generator=g)
    lab[torch.rand(lab.shape, generator=g) < 0.1] = IGNORE
    flat = lab.view(-1)
    if flat.numel() >= 4:
        flat[flat.numel() // 3] = -2
        if ld > nc:
            flat[flat.numel() // 2] = nc + (ld - nc) // 2
        flat[1] = nc - 1                               # at least one valid label
    return buf, lab


def bounds(x64, lab, s, g=None, variant=None):
    """The fp64 twin of coarse logits x64 (B, h, w, nc) (dict of tests/deepsup_fp64_twin.py: ``variant`` reaches the twin
    alone, the bounds are those of the right formulation) plus E_lse, E_row (B, H, W), E_partial (1024,), E_loss and E_dl
    (B, h, w, nc) of the module docstring, and partial (1024, 2): the exact pairs in the kernels' layout."""
    B, h, w, nc = x64.shape
    t = twin(x64, lab, s, IGNORE, g=g, variant=variant)
    r = twin(x64, lab, s, IGNORE, g=g) if variant is not None else t
    l, valid = r["lse"], r["valid"]
    A = upsample(x64.abs(), s)
    Amax = A.max(-1).values
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    Ay = A.gather(-1, safe[..., None])[..., 0]
    E_lse = U * ((nc + 8) * (l.abs() + 1.0) + 4.0 * Amax)
    E_row = torch.where(valid, E_lse + U * (4.0 * Ay + (l - r["zy"]).abs()), torch.zeros_like(l))
    rows = lab.numel()
    blk = (torch.arange(rows) // 256) % SIGMA_CE_BLOCKS
    k_sum = -(-rows // (256 * SIGMA_CE_BLOCKS)) + 10
    zero = torch.zeros(SIGMA_CE_BLOCKS, dtype=torch.float64)
    E_partial = zero.index_add(0, blk, E_row.view(-1)) + k_sum * U * zero.index_add(0, blk, r["row"].abs().view(-1))
    partial = torch.stack([zero.index_add(0, blk, t["row"].view(-1)),
                           zero.index_add(0, blk, (torch.ones_like(l) if variant == "count_all" else t["valid"].double()).view(-1))], 1)
    cnt = float(r["count"])
    E_loss = (float(E_partial.sum()) + 13 * U * float(r["row"].abs().sum())) / cnt + U * abs(float(r["loss"])) if cnt > 0 else float("nan")
    N = (2 * s) ** 2
    sm, oh = r["sm"], r["oh"]
    vm = valid[..., None].double()
    E_p = U * sm * ((nc + 11) * (r["zhat"].abs() + l.abs()[..., None] + 1.0) + 4.0 * A + 4.0 * Amax[..., None])
    T = adjoint((sm - oh).abs() * vm, h, w, s)
    E_dl = float(abs(r["g"])) * (adjoint(E_p * vm, h, w, s) + (N + 2) * U * T) + N * 2.0 ** -126
    t.update(E_lse=E_lse, E_row=E_row, E_partial=E_partial, E_loss=E_loss, E_dl=E_dl, partial=partial)
    return t


def emulate_fp32(buf, lab, s, nc, g):
    """The kernels' formulas in fp32 torch ops on the padded buffer buf (B, h, w, ld): the interpolated rows axis by axis
    with the weights of the index function, lse with the row maximum taken first,
    the row losses, the pairs in the kernels' layout and dlogits (pad columns zero) for the device scalar g."""
    f32 = torch.float32
    B, h, w, ld = buf.shape
    x = buf[..., :nc]
    Uh, Uw = interp_matrix(h, s).to(f32), interp_matrix(w, s).to(f32)

    def lerp(n, v, dim):
        """(1 - lambda) v[i0] + lambda v[i1] along `dim`: two products and an add in fp32"""
        i0, i1, lam = taps(n, s)
        shape = [1] * v.dim()
        shape[dim] = -1
        lam = lam.to(f32).view(shape)
        return (1.0 - lam) * v.index_select(dim, i0) + lam * v.index_select(dim, i1)

    z = lerp(w, lerp(h, x, 1), 2)
    m = z.max(-1).values
    l = m + torch.log(torch.exp(z - m[..., None]).sum(-1))
    valid = (lab != IGNORE) & (lab >= 0) & (lab < nc)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    row = torch.where(valid, l - z.gather(-1, safe[..., None])[..., 0], torch.zeros_like(l))
    blk = (torch.arange(lab.numel()) // 256) % SIGMA_CE_BLOCKS
    zero = torch.zeros(SIGMA_CE_BLOCKS, dtype=f32)
    partial = torch.stack([zero.index_add(0, blk, row.view(-1)), zero.index_add(0, blk, valid.to(f32).view(-1))], 1)
    e = (torch.exp(z - l[..., None]) - F.one_hot(safe, nc).to(f32)) * valid[..., None].to(f32)
    dl = torch.zeros(B, h, w, ld, dtype=f32)
    dl[..., :nc] = torch.einsum("Yi,Xj,bYXc->bijc", Uh, Uw, e) * torch.tensor(float(g), dtype=f32)
    assert l.dtype == f32 and partial.dtype == f32 and dl.dtype == f32
    return dict(lse=l, row=row, partial=partial, dl=dl, valid=valid)
