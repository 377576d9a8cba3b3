#!/usr/bin/env python3
"""Generate tests/golden/loss_focal.npz by running the REFERENCE's FocalLoss2d in float64 on the CPU.

Run in the build container only (needs the reference tree, read-only):

    python tests/golden/make_golden_focal.py

What executes is the reference's class (utils/loss_opr.py:12-23), unmodified and imported from where it lies;
``engine.logger`` (absent here) is stubbed with the standard logging module, as in make_golden_ohem.py.  The class builds
an fp32 nn.NLLLoss weight and therefore refuses fp64 inputs when weighted, so the weighted case swaps ``crit.loss`` for an
nn.NLLLoss with the case's fp64 weights (same reduction and ignore_index).  Two cases pass gamma = 0 and gamma = 3.5 on
the inputs of the plain 'mean' case: the reference ignores the argument (its exponent is the literal 2), and the three
stored losses are equal bit for bit -- asserted here and again in tests/test_focal_cpu.py.

Inputs: B = 2, 8 x 8 pixels, 5 classes, 255 = ignore on about an eighth of the pixels; seeded per case.  Stored per case:
x (2, 5, 8, 8) float64, target, gamma (as passed), reduction, weight (empty = none), loss and d loss / d x (for 'none':
of the sum of the per-pixel losses).
"""
import logging
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
IGNORE = 255
B, C, H, W = 2, 5, 8, 8

# name, seed name, gamma passed, reduction, weighted, all pixels ignored
CASES = [
    ("mean", "mean", 2, "mean", False, False),
    ("sum", "sum", 2, "sum", False, False),
    ("none", "none", 2, "none", False, False),
    ("gamma_0_passed", "mean", 0, "mean", False, False),
    ("gamma_3p5_passed", "mean", 3.5, "mean", False, False),
    ("weighted_mean", "weighted_mean", 2, "mean", True, False),
    ("no_valid", "no_valid", 2, "mean", False, True),
]


def install_stubs():
    eng = types.ModuleType("engine")
    lg = types.ModuleType("engine.logger")
    lg.get_logger = lambda *a, **k: logging.getLogger("golden_focal")
    eng.logger = lg
    sys.modules.update({"engine": eng, "engine.logger": lg})
    sys.path.insert(0, REF)


def case_inputs(seed_name, all_ignored):
    g = torch.Generator().manual_seed(zlib.crc32(("focal." + seed_name).encode()) & 0x7FFFFFFF)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2.0
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.125] = IGNORE
    if all_ignored:
        t[:] = IGNORE
    w = torch.rand(C, generator=g, dtype=torch.float64) * 2.0 + 0.1
    return x, t, w


def main():
    install_stubs()
    from utils.loss_opr import FocalLoss2d
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, seed_name, gamma, reduction, weighted, all_ignored in CASES:
        x, t, w = case_inputs(seed_name, all_ignored)
        crit = FocalLoss2d(gamma=gamma, reduction=reduction, ignore_index=IGNORE)
        if weighted:
            crit.loss = torch.nn.NLLLoss(weight=w, reduction=reduction, ignore_index=IGNORE)
        xr = x.clone().requires_grad_()
        loss = crit(xr, t.clone())
        loss.sum().backward()
        print(f"{name}: gamma passed {gamma} valid {int((t != IGNORE).sum())} loss {float(loss.detach().sum()):.12g}")
        out.update({f"{name}.x": x.numpy(), f"{name}.target": t.numpy(), f"{name}.gamma": np.float64(gamma),
                    f"{name}.reduction": np.array(reduction), f"{name}.weight": w.numpy() if weighted else np.zeros(0),
                    f"{name}.loss": loss.detach().numpy(), f"{name}.grad": xr.grad.numpy()})
    for other in ("gamma_0_passed", "gamma_3p5_passed"):
        assert out[f"{other}.loss"].tobytes() == out["mean.loss"].tobytes(), "the reference read its gamma"
        assert out[f"{other}.grad"].tobytes() == out["mean.grad"].tobytes()
    path = os.path.join(HERE, "loss_focal.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
