"""Channel-aware Mamba decoder.

Mirror of /root/reference/models/decoders/MambaDecoder.py (PatchExpand :12-30, UpsampleExpand
:33-51, FinalUpsample_X4 :76-97, Mamba_up :101-148, MambaDecoder :151-280).  deep_supervision=False is
what models/builder.py:102 selects; deep_supervision=True builds the reference's ``norm_ds`` / ``output_ds`` heads (:210-212)
and runs them on the COARSE tokens: a bias-free 1x1 convolution and a bilinear interpolation commute, so the head is a GEMM
over h_i x w_i rows and the x16 / x8 / x4 expansion acts on `num_classes` channels instead of 384 / 192 / 96.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..._launch import launch, ptr
from ...layernorm import LayerNorm
import torch.nn.functional as F

from ..encoders.vmamba import CVSSDecoderBlock


class _Up2xFn(torch.autograd.Function):
    """bilinear x2 of a contiguous channels-last tensor on the HIP gather kernels (csrc/upsample.hip)."""

    @staticmethod
    def forward(ctx, x):
        B, H, W, C = x.shape
        out = torch.empty(B, 2 * H, 2 * W, C, device=x.device, dtype=torch.float32)
        launch("sigma_upsample2x_nhwc", ptr(x), ptr(out), B, H, W, C, 0, device=x.device, what="upsample2x_nhwc")
        ctx.dims = (B, H, W, C)
        return out

    @staticmethod
    def backward(ctx, g):
        B, H, W, C = ctx.dims
        g = g.contiguous()
        dx = torch.empty(B, H, W, C, device=g.device, dtype=torch.float32)
        launch("sigma_upsample2x_nhwc", ptr(g), ptr(dx), B, H, W, C, 1, device=g.device, what="upsample2x_nhwc (adjoint)")
        return dx


def _up2(x_nhwc: torch.Tensor) -> torch.Tensor:
    """bilinear x2 (align_corners=False) on an NHWC tensor: HIP gather kernels for fp32 GPU tensors with C % 4 == 0
    (ATen's channels-last kernels are 6x / 20x off the bytes they move), F.interpolate otherwise."""
    if x_nhwc.is_cuda and x_nhwc.dtype == torch.float32 and x_nhwc.shape[-1] % 4 == 0 and x_nhwc.numel() > 0:
        return _Up2xFn.apply(x_nhwc.contiguous())
    y = F.interpolate(x_nhwc.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
    return y.permute(0, 2, 3, 1)


_INTERP = {}          # (coarse size, scale, device, dtype) -> the (size * scale, size) interpolation matrix of one axis


def interp_matrix(n: int, s: int, device, dtype=torch.float32) -> torch.Tensor:
    """U (n s, n) with U @ v = the bilinear x s interpolation (align_corners=False) of a vector of n samples:
    src = max((dst + 0.5) / s - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, n - 1), lambda = src - i0, row dst holds
    1 - lambda at i0 and lambda at i1 (both on i0 where the upper tap is clamped onto it).  Built once per key from
    element-wise ops on `device` (no host round trip, nothing without a deterministic form) and kept."""
    key = (int(n), int(s), torch.device(device), dtype)
    U = _INTERP.get(key)
    if U is None:
        num = (2 * torch.arange(n * s, device=device) + 1 - s).clamp_min(0)
        i0 = torch.div(num, 2 * s, rounding_mode="floor")
        lam = ((num - i0 * 2 * s).to(dtype) / (2 * s))[:, None]
        i1 = (i0 + 1).clamp_max(n - 1)
        col = torch.arange(n, device=device)[None, :]
        U = (col == i0[:, None]).to(dtype) * (1 - lam) + (col == i1[:, None]).to(dtype) * lam
        # not kept when built inside a graph capture (a capture records the ops, it fills nothing) or under
        # torch.inference_mode() (inference tensors, which a later training step could not save for its backward; as
        # ss2d_fused._derived): an entry built outside serves every mode
        if not (U.is_cuda and torch.cuda.is_current_stream_capturing()) and not torch.is_inference_mode_enabled():
            _INTERP[key] = U
    return U


def expand_logits(z: torch.Tensor, s: int) -> torch.Tensor:
    """Bilinear x s (align_corners=False) of channels-last logits z (B, h, w, nc) as two matmuls with the constant
    matrices of ``interp_matrix``: differentiable, and deterministic in both directions (F.interpolate's backward on the
    GPU is not).  Returns the (B, nc, h s, w s) VIEW of a channels-last result, which is how the main logits reach the
    criterion; on the GPU a class count that is no multiple of 4 is expanded at a row pitch of 4 ceil(nc / 4) floats so
    that the loss kernels take the result (pointwise.cross_entropy)."""
    B, h, w, nc = z.shape
    ld = (nc + 3) // 4 * 4 if z.is_cuda else nc
    if ld != nc:
        z = F.pad(z, (0, ld - nc))
    Uh, Uw = interp_matrix(h, s, z.device, z.dtype), interp_matrix(w, s, z.device, z.dtype)
    t = torch.matmul(Uh, z.reshape(B, h, w * ld))                      # (B, H, w ld)
    t = torch.matmul(Uw, t.reshape(B * h * s, w, ld))                  # (B H, W, ld)
    return t.view(B, h * s, w * s, ld)[..., :nc].permute(0, 3, 1, 2)


class PatchExpand(nn.Module):
    """Linear(C -> 2C), pixel-shuffle 2x2 ('b h w (p1 p2 c) -> b (h p1) (w p2) c'), LayerNorm(C/2)."""

    def __init__(self, input_resolution, dim, dim_scale=2, norm_layer=LayerNorm):
        super().__init__()
        self.input_resolution = input_resolution
        self.dim = dim
        self.expand = nn.Linear(dim, 2 * dim, bias=False) if dim_scale == 2 else nn.Identity()
        self.norm = norm_layer(dim // dim_scale)

    def forward(self, x):
        x = self.expand(x)
        B, H, W, C = x.shape
        x = x.view(B, H, W, 2, 2, C // 4).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, C // 4)
        return self.norm(x)


class UpsampleExpand(nn.Module):
    """Linear(C -> C/2), bilinear x2, LayerNorm(C/2)."""

    def __init__(self, input_resolution, dim, patch_size=4, norm_layer=LayerNorm):
        super().__init__()
        self.input_resolution = input_resolution
        self.dim = dim
        self.patch_size = patch_size
        self.linear = nn.Linear(dim, dim // 2, bias=False)
        self.output_dim = dim
        self.norm = norm_layer(dim // 2)

    def forward(self, x):
        return self.norm(_up2(self.linear(x)))


class FinalUpsample_X4(nn.Module):
    """Linear, bilinear x2, Linear, bilinear x2, LayerNorm -- back to the input resolution."""

    def __init__(self, input_resolution, dim, patch_size=4, norm_layer=LayerNorm):
        super().__init__()
        self.input_resolution = input_resolution
        self.dim = dim
        self.patch_size = patch_size
        self.linear1 = nn.Linear(dim, dim, bias=False)
        self.linear2 = nn.Linear(dim, dim, bias=False)
        self.output_dim = dim
        self.norm = norm_layer(dim)

    def forward(self, x):
        x = _up2(self.linear1(x))
        x = _up2(self.linear2(x))
        return self.norm(x)


class Mamba_up(nn.Module):
    """`depth` CVSS blocks (d_state 4) followed by an optional UpsampleExpand."""

    def __init__(self, dim, input_resolution, depth, dt_rank="auto", d_state=4, ssm_ratio=2.0, attn_drop_rate=0.0,
                 drop_rate=0.0, mlp_ratio=4.0, drop_path=0.1, norm_layer=LayerNorm, upsample=None,
                 use_checkpoint=False, **kwargs):
        super().__init__()
        self.input_resolution = input_resolution
        self.depth = depth
        rates = drop_path if isinstance(drop_path, (list, tuple)) else [drop_path] * depth
        self.blocks = nn.ModuleList([
            CVSSDecoderBlock(hidden_dim=dim, drop_path=rates[i], norm_layer=norm_layer, attn_drop_rate=attn_drop_rate,
                             d_state=d_state, dt_rank=dt_rank, ssm_ratio=ssm_ratio) for i in range(depth)])
        self.upsample = (UpsampleExpand(input_resolution, dim=dim, patch_size=2, norm_layer=norm_layer)
                         if upsample is not None else None)

    def forward(self, x):
        for blk in self.blocks:
            x = blk(x)
        return x if self.upsample is None else self.upsample(x)


class MambaDecoder(nn.Module):
    def __init__(self, img_size=(480, 640), in_channels=(96, 192, 384, 768), num_classes=40, dropout_ratio=0.1,
                 embed_dim=96, align_corners=False, patch_size=4, depths=(4, 4, 4, 4), mlp_ratio=4.0, drop_rate=0.0,
                 attn_drop_rate=0.0, drop_path_rate=0.1, norm_layer=LayerNorm, use_checkpoint=False,
                 deep_supervision=False, **kwargs):
        super().__init__()
        depths = list(depths)
        self.num_classes = num_classes
        self.num_layers = len(depths)
        self.mlp_ratio = mlp_ratio
        self.patch_size = patch_size
        self.patches_resolution = [img_size[0] // patch_size, img_size[1] // patch_size]
        self.deep_supervision = bool(deep_supervision)
        dpr = [r.item() for r in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers_up = nn.ModuleList()
        for i in range(self.num_layers):
            lvl = self.num_layers - 1 - i                         # encoder stage feeding this level
            res = (self.patches_resolution[0] // 2 ** lvl, self.patches_resolution[1] // 2 ** lvl)
            dim = int(embed_dim * 2 ** lvl)
            if i == 0:
                layer = PatchExpand(input_resolution=res, dim=dim, dim_scale=2, norm_layer=norm_layer)
            else:
                layer = Mamba_up(dim=dim, input_resolution=res, depth=depths[lvl], mlp_ratio=mlp_ratio,
                                 drop=drop_rate, attn_drop=attn_drop_rate,
                                 drop_path=dpr[sum(depths[:lvl]):sum(depths[:lvl + 1])], norm_layer=norm_layer,
                                 upsample=PatchExpand if i < self.num_layers - 1 else None,
                                 use_checkpoint=use_checkpoint)
            self.layers_up.append(layer)
        self.norm_up = norm_layer(embed_dim)
        if self.deep_supervision:                                 # MambaDecoder.py:210-212: same names, same shapes
            dims = [embed_dim * 2 ** (self.num_layers - 2 - i) for i in range(self.num_layers - 1)]
            self.norm_ds = nn.ModuleList([norm_layer(d) for d in dims])
            self.output_ds = nn.ModuleList([nn.Conv2d(d, num_classes, kernel_size=1, bias=False) for d in dims])
        self.up = FinalUpsample_X4(input_resolution=tuple(self.patches_resolution), patch_size=4, dim=embed_dim)
        self.output = nn.Conv2d(embed_dim, num_classes, kernel_size=1, bias=False)

    def forward_up_features(self, inputs, collect=None):
        """inputs: 4 fused maps (B, C_i, H_i, W_i), finest first.  `collect` (deep supervision, MambaDecoder.py:242-257): a
        list that receives norm_ds[i](y) after levels 0, 1, 2, channels-last."""
        y = self.layers_up[0](inputs[3].permute(0, 2, 3, 1))
        if collect is not None:
            collect.append(self.norm_ds[0](y))
        for i in range(1, self.num_layers):
            skip = inputs[3 - i]
            H, W = skip.shape[2], skip.shape[3]
            if y.shape[1] != H or y.shape[2] != W:               # odd sizes (PST900: 46 rows -> 45)
                y = F.interpolate(y.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
            y = self.layers_up[i](y + skip.permute(0, 2, 3, 1))
            if collect is not None and i < self.num_layers - 1:
                collect.append(self.norm_ds[i](y))
        return self.norm_up(y)

    def _head(self, x, conv):
        """the bias-free 1x1 convolution `conv` on channels-last fp32 GPU tokens x (B, H, W, C) as a GEMM: (B, H, W, nc)"""
        from ...gemm import classifier, classifier_ok, gemm_mode, linear
        if gemm_mode() == "split3" and classifier_ok(x.reshape(-1, x.shape[-1]), conv.weight):
            # a class count that is no multiple of 4 (MFNet 9, PST900 5, SUN-RGBD 37): logits at a row pitch of
            # 4 ceil(nc / 4) floats, so the classifier's three GEMMs and the loss stay on the project's kernels
            return classifier(x, conv.weight)
        w2 = conv.weight.view(conv.weight.shape[0], -1)
        return linear(x, w2) if gemm_mode() == "split3" else F.linear(x, w2)

    def up_x4(self, x, pz):
        x = self.up(x)                                            # (B, 4H, 4W, C)
        if x.is_cuda and x.dtype == torch.float32 and self.output.bias is None:
            # the 1x1 classifier (MambaDecoder.py:189, 276-280) as a GEMM over the channels-last tokens: the reference's
            # conv wants (B, C, 4H, 4W), i.e. a transposing copy of the largest activation of the model (944 MB at batch 8)
            # and a weight gradient with the strides of a (nc, C, 1, 1) view that DistributedDataParallel has to re-lay
            # (the "Grad strides do not match bucket view strides" warning of round 2).  The logits come back as a
            # (B, nc, 4H, 4W) VIEW of the channels-last result.
            return self._head(x, self.output).permute(0, 3, 1, 2)
        return self.output(x.permute(0, 3, 1, 2))

    def forward_deep(self, inputs):
        """deep supervision: (x_last, [(coarse logits (B, h_i, w_i, nc), scale_i)] for the three heads) -- output_ds[i] on
        norm_ds[i](y) at the resolution the decoder has it, with the integer scale (16, 8, 4) up to x_last's size"""
        maps = []
        x_last = self.up_x4(self.forward_up_features(inputs, collect=maps), self.patch_size)
        aux = []
        for i, m in enumerate(maps):
            if m.is_cuda and m.dtype == torch.float32:
                z = self._head(m, self.output_ds[i])
            else:
                z = F.linear(m, self.output_ds[i].weight.view(self.num_classes, -1))
            aux.append((z, self.patch_size * 2 ** (self.num_layers - 2 - i)))
        return x_last, aux

    def forward(self, inputs):
        if not self.deep_supervision:
            return self.up_x4(self.forward_up_features(inputs), self.patch_size)
        # MambaDecoder.py:264-270: (x_last, x_output_0, x_output_1, x_output_2), each (B, nc, H, W)
        x_last, aux = self.forward_deep(inputs)
        return (x_last, *(expand_logits(z, s) for z, s in aux))
