"""Fused core of SS2D (``cross_selective_scan``, reference models/encoders/vmamba.py:165-226)
as ONE autograd function around the gfx950 scan kernels.

What the reference does per SS2D call (and what autograd then mirrors in backward):
``CrossScan`` materialises 4 permuted copies of x (vmamba.py:80-98), two einsums project every
copy (x_proj, dt_proj: :193-199), 5 ``.contiguous()/.float()`` copies feed the CUDA operator
(:201-207), ``CrossMerge`` un-flips / un-transposes and adds (:100-121).

Here the four directions are never materialised:

* only TWO physical copies of x exist (row-major and column-major order); the operator reads
  them for four groups through ``u_group_shift`` and runs the two flipped directions backwards by
  addressing (``rev_group_mask``) -- include/sigma_scan.h;
* x_proj / dt_proj act point-wise along the sequence, so they are applied to the two memory
  orders in natural order (they commute with the flip); the scan reads delta / B / C of a flipped
  direction at L-1-l.  B and C are strided views of the projection output, dB / dC are written by
  the kernel straight into the gradient of that output -- no split / cat / contiguous copies;
* directions are processed in the group order [0, 2, 1, 3] (both directions of one memory order
  adjacent) so that the projection output of a stacked-weight GEMM IS the (B, G, N, L) operand;
* CrossMerge is two adds and one transposed add; its adjoint hands the SAME gradient to the two
  directions of a memory order (``dout_group_shift``) instead of four flipped copies.

Parameter layout is the reference's (x_proj_weight (4, R+2N, d), dt_projs_weight (4, d, R),
dt_projs_bias (4, d), A_logs (4d, N), Ds (4d)); the permutation to kernel group order touches only
these small tensors.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _capi
from . import gemm as _gemm
from ._handoff import claim_xz_grad_buffer
from ._launch import launch, ptr
from . import selective_scan_cuda_core as _core

# kernel group g -> reference direction k.  g = 2*j + i with j = memory order (0 row-major,
# 1 column-major) and i = flipped; reference k = j + 2*i (vmamba.py:84-89).  Self-inverse.
_PERM = (0, 2, 1, 3)
_REV_MASK = 0b1010
# bf16 pieces of the x_proj / dt_proj GEMMs on the split-operand kernels (2 / 3), 0 = the vendor fp32 batched GEMM
# (SIGMA_GEMM_XPROJ=fp32, or SIGMA_GEMM=fp32 for every GEMM of the model)
_XPROJ_ALL = os.environ.get("SIGMA_GEMM_XPROJ", "") == "all"
_XPROJ = 0 if _gemm.gemm_mode() == "fp32" else (2 if _XPROJ_ALL else _gemm._pieces("SIGMA_GEMM_XPROJ", "2"))


def _perm4(t: torch.Tensor) -> torch.Tensor:
    """t[[0, 2, 1, 3]] along dim 0 (size 4) as a strided VIEW: swapping the two middle entries of four is
    a transpose of the (2, 2) split.  Fancy indexing with a Python list builds the index tensor on the
    host and copies it to the device at every call (450 host-to-device copies + gathers per training
    step in the round-1 profile); the view costs nothing and stays on the device."""
    return t.unflatten(0, (2, 2)).transpose(0, 1).flatten(0, 1)
# One state checkpoint per backward tile (no forward sweep in the backward kernel, second-generation
# backward csrc/scan_bwd2.hip): 640-element tiles, 320 for short sequences (L = 300 pads to 320 instead of
# 640).  SIGMA_CKPT_PITCH = 0 / 320 / 640 forces one pitch for A/B runs (0 = reference-shaped x, 1280).
_CKPT_ENV = os.environ.get("SIGMA_CKPT_PITCH", "auto")


def rowlane_possible() -> bool:
    """False when SIGMA_CKPT_PITCH rules the row-lane kernels (checkpoint pitch 16) out for every launch of this process."""
    return _CKPT_ENV in ("auto", "16")


def rowlane_pays(seqlen: int, dstate: int, rows: int, groups: int) -> bool:
    """Launch shapes on which the row-lane kernels (csrc/scan_fwdr.hip / scan_bwdr.hip, checkpoint pitch 16) beat the
    quad-row / 64-lane kernels in forward + backward time, from the shape-by-shape comparison on MI355X
    (profiles/r04_rowlane_vs_auto.txt; tools/scan_bench.py --pitch 16 against the automatic choice):
      * 16 (8) states: sequences of ~1200 at any batch (the dominant launch of the training step, (16,3072,1200): 1133
        against 1339 us), and every launch with few rows (one image per GPU: (2,768,19200) 930 / 985, (2,1536,4800)
        472 / 508, (2,3072,1200) 253 / 292) -- not L = 300 (its 19 tiles do not amortise the workgroup set-up) and not
        the long sequences at batch 16 ((16,768,19200): 5915 / 5083: twelve row blocks per CU-load of sequential tiles);
      * 4 states (fusion blocks, decoder): launches with few rows -- everything the one-image step runs except L = 300
        ((1,192,19200) 146 / 450 us, (1,384,38400) 305 / 900, (1,768,19200) 259 / 498), and the single-group CroMB
        launches of the batch-8 step; with many rows the 4-state scans are bound by memory traffic, where the 64-lane
        forward is ahead."""
    if seqlen < 600:
        return False
    if dstate >= 8:
        return (600 <= seqlen <= 2400) or rows <= 8192
    return (rows <= 3072 and rows * seqlen <= 32_000_000) or (groups == 1 and rows <= 8192 and seqlen <= 2400)


def ckpt_pitch_for(seqlen: int, dstate: int = 16, rows: int = 0, quad_ok: bool = False, rowlane_ok: bool = False,
                   groups: int = 0) -> int:
    """Checkpoint pitch = backward tile length (include/sigma_scan.h).  Measured on MI355X
    (profiles/r02_bwd_plans.txt, profiles/r02_bwd4_shapes.txt, profiles/r04_rowlane_vs_auto.txt):
      * 16 (row-lane kernels, csrc/scan_fwdr.hip / scan_bwdr.hip; ``rowlane_ok`` = selective_scan_cuda_core.rowlane_ok
        of the operands) on the launch shapes ``rowlane_pays`` lists;
      * 160 (quad-row backward, csrc/scan_bwd4.hip; ``quad_ok`` = selective_scan_cuda_core.quad_backward_ok of the
        operands) whenever there are enough rows for workgroups of 8+ waves on every CU (batch * dim >= 8192 with
        8+ states; >= 12288 with 4 states up to 4800 elements, where the per-tile overhead weighs more) -- 8-27 %
        faster than the tiles below on the encoder launches (profiles/r02_bwd4_shapes.txt, r02_bwd4_mid.txt);
      * 160 as well for 8+ states, few rows and L >= 4800, where the quad-row backward splits the sequence into
        segments (csrc/scan_bwd4.hip, rev_summary4_kernel);
      * 320-element tiles for short sequences (L = 300 pads to 320 instead of 640), for 4-state scans up to 1280
        elements (state-parallel backward, csrc/scan_bwd3.hip) and for 16-state scans up to 4800 elements with
        enough rows for the row-block loop of csrc/scan_bwd2.hip;
      * 640 otherwise."""
    if _CKPT_ENV not in ("auto", "norowlane"):
        forced = int(_CKPT_ENV)
        if (forced != 160 or quad_ok) and (forced != 16 or rowlane_ok):
            return forced
    if rowlane_ok and _CKPT_ENV != "norowlane" and rowlane_pays(seqlen, dstate, rows, groups):
        return 16
    if quad_ok and ((dstate >= 8 and rows >= 8192) or (rows >= 12288 and seqlen <= 4800)):
        return 160
    if quad_ok and dstate >= 8 and seqlen >= 4800:
        # few rows, long sequences (one image per GPU, sigma_base 720x1280): the quad-row backward cuts the sequence
        # into segments run by different workgroups (profiles/r02_bwd4_segments.txt: (1,768,19200) 1081 -> 504 us,
        # (2,1024,57600) 4249 -> 2209 us); the forward stays on the 64-lane kernel, which writes the 160-pitch checkpoints
        return 160
    if seqlen <= 320 or (dstate <= 4 and seqlen <= 1280):
        return 320
    if dstate > 8 and seqlen <= 4800 and rows >= 12288:
        return 320
    return 640


def _two_orders(x4: torch.Tensor) -> torch.Tensor:
    """(B, d, H, W) -> (B, 2, d, L): [row-major, column-major] sequences of the same image."""
    B, d, H, W = x4.shape
    out = x4.new_empty(B, 2, d, H * W)
    out[:, 0].view(B, d, H, W).copy_(x4)
    out[:, 1].view(B, d, W, H).copy_(x4.transpose(2, 3))
    return out


def _planes_ok(x: torch.Tensor) -> bool:
    """(B, d, H, W) whose H x W planes are contiguous and do not overlap: the packed tensor, or the permuted view of a
    channel-major (d, B, H, W) buffer (include/sigma_ops.h, x_batch_stride / x_channel_stride)"""
    if x.dim() != 4:
        return False
    B, d, H, W = x.shape
    L = H * W
    sb, sc, sh, sw = x.stride()
    if (sh, sw) != (W, 1) and L > 1:
        return False
    if x.data_ptr() % 16:
        return False
    return (sb, sc) == (d * L, L) or (sc == B * L and sb == L) or (B == 1 and sc >= L) or (d == 1 and sb >= L)


class DwConvSiLUTwoOrdersFn(torch.autograd.Function):
    """xs2 = [silu(dwconv3x3(x)) row-major, the same column-major]  (B, d, H, W) -> (B, 2, d, H*W).

    Reference: SS2D.forward vmamba.py:1071-1072 + the layout half of CrossScan (:80-89); kernels in
    sigma_amd/csrc/dwconv.hip, C ABI in include/sigma_ops.h."""

    @staticmethod
    def forward(ctx, x, weight, bias, n_orders=2):
        if not x.is_cuda:
            raise RuntimeError("dwconv3x3_silu: GPU tensors only (no fallback)")
        x = x.float()
        if not _planes_ok(x):
            x = x.contiguous()
        w = weight.float().contiguous()
        b = None if bias is None else bias.float().contiguous()
        B, d, H, W = x.shape
        if tuple(w.shape) != (d, 1, 3, 3):
            raise RuntimeError("dwconv3x3_silu: weight must be (d, 1, 3, 3)")
        out2 = torch.empty(B, n_orders, d, H * W, device=x.device, dtype=torch.float32)
        ctx.n_orders = n_orders
        p = _capi.DwConvParams()
        p.batch, p.channels, p.height, p.width, p.n_orders = B, d, H, W, n_orders
        p.x, p.weight, p.bias, p.out2 = x.data_ptr(), w.data_ptr(), (b.data_ptr() if b is not None else None), out2.data_ptr()
        p.x_batch_stride, p.x_channel_stride = x.stride(0), x.stride(1)
        launch("sigma_dwconv3x3_silu_fwd", ctypes.byref(p), device=x.device, what="dwconv3x3_silu_fwd")
        ctx.save_for_backward(x, w, b if b is not None else x.new_empty(0))
        ctx.has_bias = b is not None
        return out2

    @staticmethod
    def backward(ctx, g2):
        x, w, b = ctx.saved_tensors
        B, d, H, W = x.shape
        g2 = g2.float().contiguous()
        gpre = torch.empty(B, d, H, W, device=x.device, dtype=torch.float32)
        # dx in the layout of x: the channel-major (d, B, H, W) buffer of the in_proj hand-over stays channel-major, so that
        # LinearXZFn.backward reads it in place (gemm.py)
        dx = torch.empty_strided(x.shape, x.stride(), device=x.device, dtype=torch.float32)
        # deterministic mode (sigma_amd/deterministic.py): dweight / dbias are written through a fixed-order two-stage sum
        det = torch.are_deterministic_algorithms_enabled()
        alloc = torch.empty if det else torch.zeros
        dw = alloc(w.shape, device=w.device, dtype=w.dtype)
        db = alloc(d, device=x.device, dtype=torch.float32) if ctx.has_bias else None
        p = _capi.DwConvParams()
        p.batch, p.channels, p.height, p.width, p.n_orders = B, d, H, W, ctx.n_orders
        p.flags = _capi.SIGMA_DWCONV_DETERMINISTIC if det else 0
        p.x, p.weight, p.bias = x.data_ptr(), w.data_ptr(), (b.data_ptr() if ctx.has_bias else None)
        p.g2, p.gpre, p.dweight, p.dx = g2.data_ptr(), gpre.data_ptr(), dw.data_ptr(), dx.data_ptr()
        p.x_batch_stride, p.x_channel_stride = x.stride(0), x.stride(1)
        p.dbias = db.data_ptr() if db is not None else None
        workspace = None
        if det:
            ws_bytes = int(_capi.load().sigma_dwconv3x3_silu_bwd_workspace_bytes(ctypes.byref(p)))
            if ws_bytes < 0:
                raise RuntimeError("dwconv3x3_silu_bwd: invalid sizes")
            workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
            p.workspace, p.workspace_bytes = workspace.data_ptr(), ws_bytes
        launch("sigma_dwconv3x3_silu_bwd", ctypes.byref(p), device=x.device, what="dwconv3x3_silu_bwd")
        return dx, dw, db, None


def dwconv_silu_two_orders(x, weight, bias):
    return DwConvSiLUTwoOrdersFn.apply(x, weight, bias, 2)


def dwconv_silu(x, weight, bias):
    """silu(depthwise conv3x3(x) + bias), (B, d, H, W) -> (B, d, H, W); HIP kernel, GPU tensors only."""
    B, d, H, W = x.shape
    return DwConvSiLUTwoOrdersFn.apply(x, weight, bias, 1).view(B, d, H, W)


def _transpose2d(src, dst, B, R, C, src_bs, src_rs, dst_bs, dst_rs):
    p = _capi.TransposeParams()
    p.batch, p.rows, p.cols = B, R, C
    p.src, p.dst = src.data_ptr(), dst.data_ptr()
    p.src_batch_stride, p.src_row_stride, p.dst_batch_stride, p.dst_row_stride = src_bs, src_rs, dst_bs, dst_rs
    launch("sigma_transpose2d", ctypes.byref(p), device=src.device, what="transpose2d")


class SplitXZFn(torch.autograd.Function):
    """xz (B, H, W, 2d) -> (x channels-first (B, d, H, W) contiguous, z = the view xz[..., d:]).

    Reference: ``x, z = xz.chunk(2, dim=-1); x = x.permute(0, 3, 1, 2).contiguous()`` (vmamba.py:1070-1071).
    Forward is one tiled transpose reading the x half in place; backward writes dx (channels-first) into
    the x half of ONE gradient buffer with the inverse transpose and copies dz into the z half, instead
    of autograd's strided cat of a permuted view."""

    @staticmethod
    def forward(ctx, xz):
        B, H, W, d2 = xz.shape
        d, L = d2 // 2, H * W
        xz = xz.contiguous()
        x = torch.empty(B, d, H, W, device=xz.device, dtype=xz.dtype)
        _transpose2d(xz, x, B, L, d, L * d2, d2, d * L, L)
        ctx.dims = (B, H, W, d)
        z = xz[..., d:]
        return x, z

    @staticmethod
    def backward(ctx, dx, dz):
        B, H, W, d = ctx.dims
        L = H * W
        dxz = claim_xz_grad_buffer(dz, (B, H, W, 2 * d)) if (dz is not None and dz.dtype == dx.dtype) else None
        if dxz is None:                   # else: the gated LayerNorm's backward wrote dz into the z half already (layernorm.py)
            dxz = torch.empty(B, H, W, 2 * d, device=dx.device, dtype=dx.dtype)
            if dz is None:
                dxz[..., d:].zero_()
            else:
                dxz[..., d:].copy_(dz)
        _transpose2d(dx.contiguous(), dxz, B, d, L, d * L, L, L * 2 * d, 2 * d)
        return dxz


def split_xz(xz):
    return SplitXZFn.apply(xz)


class SelectiveScanExtFn(torch.autograd.Function):
    """selective scan with the operator extensions of include/sigma_scan.h under autograd:
    ``rev_mask`` (bit g: group g runs backwards by addressing) and ``u_gshift`` (group g reads the
    u rows of group g >> u_gshift; u is (B, dim >> u_gshift, L)).  Used by ConMB, whose two
    directions are the concatenated RGB|X sequence and its flip (vmamba.py:123-163, 369-430)."""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, delta_bias, rev_mask, u_gshift, pair_sum=False):
        u, delta = u.float().contiguous(), delta.float().contiguous()
        B = B.float() if B.stride(-1) == 1 else B.float().contiguous()
        C = C.float() if C.stride(-1) == 1 else C.float().contiguous()
        A, D, delta_bias = A.float().contiguous(), D.float().contiguous(), delta_bias.float().contiguous()
        pitch = ckpt_pitch_for(u.shape[-1], A.shape[1], delta.shape[0] * delta.shape[1], _core.quad_backward_ok(u, delta, B, C),
                               _core.rowlane_ok(u, delta, B, C), B.shape[1])
        out, ck = _core.fwd_ext(u, delta, A, B, C, D, delta_bias, True, rev_mask=rev_mask, u_gshift=u_gshift,
                                need_x=any(ctx.needs_input_grad), ckpt_pitch=pitch)
        ctx.save_for_backward(u, delta, A, B, C, D, delta_bias, ck)
        ctx.ext = (int(rev_mask), int(u_gshift), bool(pair_sum))
        ctx.pitch = pitch                                     # the backward tile IS the forward's checkpoint pitch
        if pair_sum:
            # y = group 0 + group 1 (ConMB's CrossMerge, vmamba.py:151-157).  Summed HERE so that the backward hands the
            # ONE gradient to both groups through dout_group_shift instead of autograd's two zero-filled (B, 2, d, L)
            # buffers, two strided copies and an add (SelectBackward0: 1.0 ms per step)
            Bsz, dim, L = out.shape
            if B.shape[1] != 2:
                raise RuntimeError("pair_sum: two groups only")
            o4 = out.view(Bsz, 2, dim // 2, L)
            return o4[:, 0] + o4[:, 1]
        return out

    @staticmethod
    def backward(ctx, dout):
        u, delta, A, B, C, D, delta_bias, ck = ctx.saved_tensors
        rev_mask, sh, pair_sum = ctx.ext
        dout = dout.float()
        if dout.stride(-1) != 1:
            dout = dout.contiguous()
        du, ddelta, dA, dB, dC, dD, dbias = _core.bwd_ext(u, delta, A, B, C, D, delta_bias, dout, ck,
                                                          True, rev_mask=rev_mask, u_gshift=sh, dout_gshift=1 if pair_sum else 0,
                                                          ckpt_pitch=ctx.pitch)
        if sh:
            Bsz, dim, L = du.shape
            G = B.shape[1]
            rpg = dim // G
            du = du.view(Bsz, G >> sh, 1 << sh, rpg, L).sum(2).reshape(Bsz, dim >> sh, L)
        # dA / dD / dbias are views of ONE zero-filled buffer (bwd_ext): hand autograd tensors that own their storage
        return du, ddelta, dA.clone(), dB, dC, dD.clone(), dbias.clone(), None, None, None


def selective_scan_ext(u, delta, A, B, C, D, delta_bias, rev_mask=0, u_gshift=0, pair_sum=False):
    return SelectiveScanExtFn.apply(u, delta, A, B, C, D, delta_bias, rev_mask, u_gshift, pair_sum)


def _merge_params(B, d, H, W):
    p = _capi.MergeParams()
    p.batch, p.channels, p.height, p.width = B, d, H, W
    return p


def cross_merge_nhwc(ys: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """(B, 4, d, L) scan planes (group order g = 2*order + flipped, natural positions) -> (B, H, W, d)."""
    B, _, d, L = ys.shape
    y = torch.empty(B, H, W, d, device=ys.device, dtype=torch.float32)
    p = _merge_params(B, d, H, W)
    p.planes4, p.nhwc = ys.data_ptr(), y.data_ptr()
    launch("sigma_cross_merge_nhwc", ctypes.byref(p), device=ys.device, what="cross_merge_nhwc")
    return y


def cross_split_nhwc(dy: torch.Tensor) -> torch.Tensor:
    """(B, H, W, d) -> (B, 2, d, L): the gradient once in row-major and once in column-major order."""
    B, H, W, d = dy.shape
    g2 = torch.empty(B, 2, d, H * W, device=dy.device, dtype=torch.float32)
    p = _merge_params(B, d, H, W)
    p.planes2, p.nhwc = g2.data_ptr(), dy.data_ptr()
    launch("sigma_cross_split_nhwc", ctypes.byref(p), device=dy.device, what="cross_split_nhwc")
    return g2


def _pair_sum_add(src: torch.Tensor, acc: torch.Tensor, n_outer: int, inner: int) -> None:
    """acc (n_outer, inner) += src (n_outer, 2, inner).sum(1), one HIP pass (include/sigma_ops.h)."""
    if not (src.is_contiguous() and acc.is_contiguous() and src.dtype == torch.float32 and acc.dtype == torch.float32):
        raise RuntimeError("pair_sum_add: contiguous fp32 tensors only")
    launch("sigma_pair_sum_add", ptr(src), ptr(acc), n_outer, inner, device=src.device, what="pair_sum_add")


# Tensors derived from the SS2D parameters alone (permuted / stacked / transposed weight copies, A = -exp(A_logs)): a
# handful of tiny launches per block and step.  They are cached per parameter VERSION: the key is
# the parameters' storage addresses and autograd version counters (every in-place update -- optimizer step,
# load_state_dict, copy_ -- bumps the counter; ``p.data = ...`` changes the address), the entry holds a weak reference to
# the parameter object it was built from; optimizer steps drop the entries of the parameters they own (the fused
# optimizers do not bump version counters).  Never inside a stream capture: a replayed graph runs no Python, so a captured
# step must contain the derivation kernels themselves (parameters stepped by a captured optimizer would otherwise be
# read through stale copies).  NOT seen by the key: in-place writes through ``param.data`` (a detached alias with its own
# version counter) -- code that updates these parameters that way calls ``invalidate_derived_params()`` afterwards, or
# runs with SIGMA_CACHE_DERIVED=0 (rebuild on every call, the behaviour up to round 3).
_DERIVED = {}
_CACHE_DERIVED = os.environ.get("SIGMA_CACHE_DERIVED", "1") != "0"


def invalidate_derived_params() -> None:
    """drop every cached parameter-derived tensor (after in-place writes through ``param.data``)"""
    _DERIVED.clear()


def _after_optimizer_step(optimizer, args, kwargs) -> None:
    """Optimizer post-step hook: the fused ("single kernel") optimizers update parameters WITHOUT bumping their version
    counters (torch.optim.AdamW(fused=True): measured), so a step drops the entries built from any parameter the
    optimizer owns.  The reference's groups leave the raw Mamba parameters out (utils/init_func.py:33-58): for its step
    nothing is dropped and the cache lives across steps.  Reads the optimizer, never writes to it."""
    if not _DERIVED:
        return
    owned = {id(q) for g in optimizer.param_groups for q in g["params"]}
    for k in [k for k, ent in _DERIVED.items() if any(i in owned for i in ent[3])]:
        _DERIVED.pop(k, None)


_HOOK = {"state": None}                           # None: not tried yet; True: registered; False: this torch has no global hooks


def _ensure_step_hook() -> bool:
    """Registers the global optimizer hook the FIRST time an entry is about to be cached -- importing the package has no
    process-wide side effect, and a process that never caches (SIGMA_CACHE_DERIVED=0, captured steps) never gets one."""
    if _HOOK["state"] is None:
        try:
            from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_post
            _reg_post(_after_optimizer_step)
            _HOOK["state"] = True
        except Exception:                         # a torch without global optimizer hooks: no caching at all
            _HOOK["state"] = False
    return _HOOK["state"]


def _derived_params(x_proj_weight, dt_projs_weight, A_logs):
    """(Wst (2, 2c, d), Wst^T (2, d, 2c), dtw (4, d, R), A (4d, N)) in the kernels' group order, fp32, contiguous"""
    import weakref

    def build():
        K, c, d = x_proj_weight.shape
        Wst = _perm4(x_proj_weight.detach().float()).reshape(2, 2 * c, d).contiguous()   # [order j][(flip i, row)][d]
        dtw = _perm4(dt_projs_weight.detach().float()).contiguous()                       # (4, d, R)
        A = -torch.exp(A_logs.detach().float())
        return Wst, Wst.transpose(1, 2).contiguous(), dtw, A

    if not _CACHE_DERIVED or (x_proj_weight.is_cuda and torch.cuda.is_current_stream_capturing()) or not _ensure_step_hook():
        return build()
    key = (x_proj_weight.data_ptr(), x_proj_weight._version, dt_projs_weight.data_ptr(), dt_projs_weight._version,
           A_logs.data_ptr(), A_logs._version)
    ent = _DERIVED.get(id(x_proj_weight))
    if ent is not None and ent[0] == key and ent[1]() is x_proj_weight:
        return ent[2]
    val = build()
    if torch.is_inference_mode_enabled():
        # built under torch.inference_mode(): inference tensors, which a later training forward could not save for its
        # backward (an evaluation between two training steps would leave them behind: the reference's optimizer steps
        # none of these parameters, so nothing drops the entry).  Not cached; an entry built outside serves both.
        return val
    if len(_DERIVED) > 4096:                     # parameters that died without a lookup: start over
        _DERIVED.clear()
    _DERIVED[id(x_proj_weight)] = (key, weakref.ref(x_proj_weight), val, (id(x_proj_weight), id(dt_projs_weight), id(A_logs)))
    return val


class SS2DCoreFn(torch.autograd.Function):
    """y = CrossMerge(selective_scan(CrossScan(x), ...)); input xs2 = [row-major, column-major]
    sequences of x, (B, 2, d, H*W) -> y channels-last (B, H, W, d), ready for out_norm."""

    @staticmethod
    def forward(ctx, xs2, H, W, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds):
        B, _, d, L = xs2.shape
        if L != H * W:
            raise RuntimeError("SS2DCoreFn: xs2 must be (B, 2, d, H*W)")
        K, c, _ = x_proj_weight.shape
        R = dt_projs_weight.shape[2]
        N = A_logs.shape[1]
        if K != 4:
            raise RuntimeError("SS2DCoreFn expects the 4-direction parameter stack")
        xs2 = xs2.float().contiguous()
        Wst, WstT, dtw, A = _derived_params(x_proj_weight, dt_projs_weight, A_logs)
        # The projections on the split-operand MFMA kernels (stacked problems, weight stacks shared through a_mod, no
        # expanded weight copies, results written straight into their slices, weight gradients summed over the batch
        # inside the kernel) WHERE THEY BEAT the vendor fp32 batched GEMM + its helper passes -- measured per GEMM and
        # stage in profiles/r04_xproj_bench.txt (tools/xproj_bench.py): x_proj forward and its input gradient (with the
        # scan's two du as epilogue addends: no pair-sum pass) everywhere, its weight gradient and dt_proj up to L = 1200,
        # dt_proj's weight gradient on the last stage only, dt_proj's input gradient (M = dt_rank) nowhere.  SIGMA_GEMM_XPROJ=fp32 (or a reduction
        # length that is not a multiple of 4: dt_rank 6 of the 96-channel stage) keeps the vendor GEMMs; =all takes
        # every GEMM the kernels can (A/B runs).
        legal = bool(_XPROJ) and L % 4 == 0 and d % 4 == 0 and c % 2 == 0
        short = L <= 600 or _XPROJ_ALL
        mid = L <= 1200 or _XPROJ_ALL
        own_x = legal
        own_dt = legal and R % 4 == 0 and mid
        ctx.own = dict(xd=legal, xw=legal and mid, dd=legal and R % 4 == 0 and _XPROJ_ALL, dw=legal and R % 4 == 0 and short)
        if own_x:
            p4 = torch.empty((B, 4, c, L), device=xs2.device, dtype=torch.float32)
            _gemm.bgemm_nn(Wst, xs2.view(2 * B, d, L), p4.view(2 * B, 2 * c, L), pieces=_XPROJ)
        else:
            p4 = torch.matmul(Wst.unsqueeze(0), xs2).view(B, 4, c, L)          # == (B, group g, R+2N, L)
        if own_dt:
            delta = torch.empty((B, 4, d, L), device=xs2.device, dtype=torch.float32)
            _gemm.bgemm_nn(dtw, p4.view(4 * B, c, L)[:, :R], delta.view(4 * B, d, L), pieces=_XPROJ)
        else:
            delta = torch.matmul(dtw.unsqueeze(0), p4[:, :, :R])               # (B, 4, d, L)
        # A, D, bias keep the reference's direction order: the kernels map group -> parameter rows (param_swap)
        Dp = Ds.float()
        bias = dt_projs_bias.float().reshape(-1)
        Bv, Cv = p4[:, :, R:R + N], p4[:, :, R + N:]
        need_x = any(ctx.needs_input_grad)
        u2, dl2 = xs2.view(B, 2 * d, L), delta.view(B, 4 * d, L)
        pitch = ckpt_pitch_for(L, N, B * 4 * d, _core.quad_backward_ok(u2, dl2, Bv, Cv), _core.rowlane_ok(u2, dl2, Bv, Cv), 4)
        out, ck = _core.fwd_ext(u2, dl2, A, Bv, Cv, Dp, bias, True, rev_mask=_REV_MASK, u_gshift=1, need_x=need_x,
                                ckpt_pitch=pitch, param_swap=1)
        ctx.pitch = pitch
        y = cross_merge_nhwc(out.view(B, 4, d, L), H, W)                       # (B, H, W, d)
        ctx.save_for_backward(xs2, p4, delta, A, Dp, bias, ck, Wst, dtw, WstT)
        ctx.dims = (B, d, H, W, c, R, N)
        return y

    @staticmethod
    def backward(ctx, dy):
        xs2, p4, delta, A, Dp, bias, ck, Wst, dtw, WstT = ctx.saved_tensors
        B, d, H, W, c, R, N = ctx.dims
        own = ctx.own
        L = H * W
        g2 = cross_split_nhwc(dy.float().contiguous())                         # CrossMerge^T: 2 planes, not 4
        dp4 = torch.empty_like(p4)
        Bv, Cv = p4[:, :, R:R + N], p4[:, :, R + N:]
        du, ddelta, dA, _, _, dD, dbias = _core.bwd_ext(
            xs2.view(B, 2 * d, L), delta.view(B, 4 * d, L), A, Bv, Cv, Dp, bias, g2.view(B, 2 * d, L), ck, True,
            rev_mask=_REV_MASK, u_gshift=1, dout_gshift=1, dB_out=dp4[:, :, R:R + N], dC_out=dp4[:, :, R + N:], param_swap=1,
            ckpt_pitch=ctx.pitch)
        ddelta4 = ddelta.view(B, 4, d, L)
        # weight gradients computed by the kernels: the sum over the batch in two stages inside the library (no zero fill)
        wg = torch.empty(4 * d * R + 4 * c * d, device=xs2.device, dtype=torch.float32) if (own["xw"] or own["dw"]) else None
        # dt_proj: delta = dtw @ p4[:R]
        if own["dd"]:
            _gemm.bgemm_nn(dtw.transpose(1, 2).contiguous(), ddelta.view(4 * B, d, L), dp4.view(4 * B, c, L)[:, :R], pieces=_XPROJ)
        else:
            dp4[:, :, :R] = torch.matmul(dtw.transpose(1, 2).unsqueeze(0), ddelta4)
        if own["dw"]:
            d_dtw = wg[:4 * d * R].view(4, d, R)
            _gemm.bgemm_nt_sum(ddelta.view(4 * B, d, L), p4.view(4 * B, c, L)[:, :R], d_dtw, pieces=_XPROJ, accumulate=False)
        else:
            d_dtw = torch.matmul(ddelta4, p4[:, :, :R].transpose(-1, -2)).sum(0)   # (4, d, R)
        # x_proj: p = Wst @ xs2; its input gradient joins the scan's du of both directions of an order
        dp2 = dp4.view(B, 2, 2 * c, L)
        if own["xd"]:
            dxs2 = torch.empty((B, 2, d, L), device=xs2.device, dtype=torch.float32)
            du3 = du.view(2 * B, 2, d, L)
            _gemm.bgemm_nn(WstT, dp4.view(2 * B, 2 * c, L), dxs2.view(2 * B, d, L),
                           residual=du3[:, 0], residual2=du3[:, 1], pieces=_XPROJ)
        else:
            dxs2 = torch.matmul(WstT.unsqueeze(0), dp2)                        # (B, 2, d, L)
            _pair_sum_add(du, dxs2, B * 2, d * L)                              # + du of both directions of an order
        if own["xw"]:
            dWst = wg[4 * d * R:].view(2, 2 * c, d)
            _gemm.bgemm_nt_sum(dp4.view(2 * B, 2 * c, L), xs2.view(2 * B, d, L), dWst, pieces=_XPROJ, accumulate=False)
        else:
            dWst = torch.matmul(dp2, xs2.transpose(-1, -2)).sum(0)             # (2, 2c, d)
        d_xproj = _perm4(dWst.view(4, c, d))                                   # the permutation is its own inverse
        d_dtw = _perm4(d_dtw)
        dA_logs = dA * A                                                       # A = -exp(A_logs); reference order already
        dDs = dD.clone()                                                       # dD / dbias: views of one shared buffer
        dbias = dbias.clone().view(4, d)
        return dxs2, None, None, d_xproj, d_dtw, dbias, dA_logs, dDs


class _TwoOrdersFn(torch.autograd.Function):
    """(B, d, H, W) -> (B, 2, d, L) and its adjoint, with plain copies (callers without the fused conv)."""

    @staticmethod
    def forward(ctx, x):
        ctx.hw = x.shape[2:]
        return _two_orders(x.float())

    @staticmethod
    def backward(ctx, g):
        H, W = ctx.hw
        B, _, d, L = g.shape
        return g[:, 0].reshape(B, d, H, W) + g[:, 1].reshape(B, d, W, H).transpose(2, 3)


def ss2d_core(x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds):
    """x (B, d, H, W) -> (B, H, W, d)"""
    B, d, H, W = x.shape
    return SS2DCoreFn.apply(_TwoOrdersFn.apply(x), H, W, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds)


def ss2d_core_from_orders(xs2, H, W, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds):
    """xs2 (B, 2, d, H*W) as produced by dwconv_silu_two_orders -> (B, H, W, d)"""
    return SS2DCoreFn.apply(xs2, H, W, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds)
