#!/usr/bin/env python3
"""Generate block-level golden fixtures by running the REFERENCE's own blocks on CPU.

Run in the build container only (needs the reference tree, read-only):

    python tests/golden/make_golden_blocks.py

What executes is the reference's code, unmodified and imported from where it lies (models/encoders/vmamba.py:
VSSBlock, CrossMambaFusionBlock, ConcatMambaFusionBlock, CVSSDecoderBlock, PatchMerging2D), under the stubs of
make_golden_model.py (``selective_scan_cuda_core`` = the reference's ``selective_scan_ref``).  The one addition is a
DropPath stub that applies GIVEN per-sample factors (timm semantics with scale_by_keep: mask / keep probability), so
that training mode is reproducible without timm's random draw.

Weights: tests/golden/fill.py by state_dict name.  Inputs, output gradients: seeded by the case name.
Outputs: tests/golden/block_<case>.npz with the inputs, the output gradients, the factors, every output, input
gradient and parameter gradient (float32) -- the anchor of tests/block_fp64_twin.py (tests/test_blocks_fp64_cpu.py).
"""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fill  # noqa: E402
import make_golden_model  # noqa: E402

KEEP = 0.6            # drop_path = 0.4

# name, kind, reference class, (B, H, W, C), d_state, per-mask factors in units of 1 / KEEP (None: eval mode)
CASES = [
    ("vss_eval", "vss", "VSSBlock", (2, 5, 6, 32), 16, None),
    ("vss_train", "vss", "VSSBlock", (2, 5, 6, 32), 16, [[0, 1]]),
    ("cromb_eval", "cromb", "CrossMambaFusionBlock", (2, 5, 6, 32), 4, None),
    ("cromb_train", "cromb", "CrossMambaFusionBlock", (2, 5, 6, 32), 4, [[0, 1], [1, 0]]),
    ("conmb_eval", "conmb", "ConcatMambaFusionBlock", (2, 5, 6, 32), 4, None),
    ("conmb_train", "conmb", "ConcatMambaFusionBlock", (2, 5, 6, 32), 4, [[1, 0]]),
    ("cvss_eval", "cvss", "CVSSDecoderBlock", (2, 5, 6, 64), 4, None),
    ("merge_odd", "merge", "PatchMerging2D", (2, 5, 7, 32), 0, None),
]


class GivenDropPath(torch.nn.Module):
    """x * factors[b] in training mode (factors = mask / keep probability, set by the caller), identity otherwise.
    ``factors``: one (B,) tensor applied at every call, or a list with one (B,) tensor per call of a step -- the reference's
    encoder calls each of its DropPath modules twice per step, in its RGB pass and in its X pass.  ``calls`` counts the
    training-mode calls; whoever hands in a list resets it before each step."""

    def __init__(self, drop_prob=0.0, scale_by_keep=True):
        super().__init__()
        self.drop_prob = drop_prob
        self.factors = None
        self.calls = 0

    def forward(self, x):
        if not self.training:
            return x
        call, self.calls = self.calls, self.calls + 1
        if self.factors is None:
            return x
        f = self.factors[call] if isinstance(self.factors, (list, tuple)) else self.factors
        return x * f.to(x.dtype).reshape(-1, *([1] * (x.dim() - 1)))


def case_tensors(name, kind, shape):
    g = torch.Generator().manual_seed(zlib.crc32(name.split("_")[0].encode()) & 0x7FFFFFFF)
    B, H, W, C = shape
    n_in = 2 if kind in ("cromb", "conmb") else 1
    n_out = 2 if kind == "cromb" else 1
    oshape = (B, (H + 1) // 2, (W + 1) // 2, 2 * C) if kind == "merge" else shape
    return ([torch.randn(shape, generator=g) for _ in range(n_in)], [torch.randn(oshape, generator=g) for _ in range(n_out)])


def main():
    make_golden_model.install_stubs()
    sys.modules["timm.models.layers"].DropPath = GivenDropPath
    os.chdir("/tmp")
    import models.encoders.vmamba as ref
    for name, kind, cls, shape, d_state, masks in CASES:
        C = shape[-1]
        torch.manual_seed(0)
        if kind == "merge":
            blk = ref.PatchMerging2D(C, 2 * C, norm_layer=torch.nn.LayerNorm)
        elif kind in ("vss", "cvss"):
            blk = getattr(ref, cls)(hidden_dim=C, drop_path=1.0 - KEEP, norm_layer=torch.nn.LayerNorm, attn_drop_rate=0.0,
                                    d_state=d_state, dt_rank="auto", ssm_ratio=2.0, mlp_ratio=0.0)
        else:
            blk = getattr(ref, cls)(hidden_dim=C, drop_path=1.0 - KEEP, mlp_ratio=0.0, d_state=d_state)
        fill.fill_parameters(blk)
        blk.train(masks is not None)
        factors = None
        if masks is not None:
            factors = torch.tensor(masks, dtype=torch.float32) / KEEP
            dps = [m for m in blk.modules() if isinstance(m, GivenDropPath)]
            assert len(dps) == len(masks), (name, len(dps))
            for dp, f in zip(dps, factors):
                dp.factors = f
        xs, gys = case_tensors(name, kind, shape)
        xs = [x.requires_grad_() for x in xs]
        outs = blk(*xs)
        outs = outs if isinstance(outs, tuple) else (outs,)
        torch.autograd.backward(outs, gys)
        blob = {"meta": np.array(repr(dict(name=name, kind=kind, shape=shape, d_state=d_state))),
                "factors": (factors.numpy() if factors is not None else np.zeros((0, shape[0]), np.float32))}
        for i, x in enumerate(xs):
            blob[f"x{i}"], blob[f"dx{i}"] = x.detach().numpy(), x.grad.numpy()
        for i, (o, gy) in enumerate(zip(outs, gys)):
            blob[f"out{i}"], blob[f"gy{i}"] = o.detach().numpy(), gy.numpy()
        names = []
        for n, p in blk.named_parameters():
            assert p.grad is not None, n
            names.append(n)
            blob["g:" + n] = p.grad.to(torch.float32).numpy()
        assert sorted(names) == sorted(blk.state_dict().keys())                 # no buffers: fill.py rebuilds every weight
        blob["param_names"] = np.array(names)
        path = os.path.join(HERE, f"block_{name}.npz")
        np.savez_compressed(path, **blob)
        print(path, [tuple(o.shape) for o in outs], "%.0f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
