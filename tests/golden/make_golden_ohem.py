#!/usr/bin/env python3
"""Generate tests/golden/loss_ohem.npz by running the REFERENCE's ProbOhemCrossEntropy2d in float64 on the CPU.

Run in the build container only (needs the reference tree, read-only):

    python tests/golden/make_golden_ohem.py

What executes is the reference's class (utils/loss_opr.py:137-187), unmodified and imported from where it lies.  Two
stand-ins make it run: ``engine.logger`` (absent here) is stubbed with the standard logging module, and
``Tensor.__rsub__`` is given a boolean case -- the class inverts its masks with ``1 - mask``, which current torch refuses
for bool tensors; ``1 - mask`` then means ``~mask``, what it meant when the class was written.  The class has no weight
argument of its own table for other datasets, so the weighted case swaps the criterion it holds for one with the case's
weights (same reduction and ignore_index).

Inputs: B = 2, 8 x 8 pixels, 5 classes, 255 = ignore on about an eighth of the pixels; seeded per case.  Stored per case:
x (2, 5, 8, 8) float64, target, thresh, min_kept, reduction, weight (empty = none), loss and d loss / d x.  The kept
pixels are those with a non-zero gradient row.
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

# name, thresh, min_kept (an int, or "valid+1" / "valid"), reduction, weighted, all pixels ignored, plant a tie at rank k
CASES = [
    ("thresh_governs", 0.7, 8, "mean", False, False, False),
    ("kth_governs", 0.05, 60, "mean", False, False, False),
    ("kth_governs_tie", 0.05, 70, "mean", False, False, True),
    ("more_than_valid", 0.3, "valid+1", "mean", False, False, False),
    ("equal_valid", 0.3, "valid", "mean", False, False, False),
    ("zero_min_kept", 0.3, 0, "mean", False, False, False),
    ("no_valid", 0.3, 10, "mean", False, True, False),
    ("weighted_mean", 0.3, 40, "mean", True, False, False),
    ("sum", 0.5, 30, "sum", False, False, False),
]


def install_stubs():
    eng = types.ModuleType("engine")
    lg = types.ModuleType("engine.logger")
    lg.get_logger = lambda *a, **k: logging.getLogger("golden_ohem")
    eng.logger = lg
    sys.modules.update({"engine": eng, "engine.logger": lg})
    sys.path.insert(0, REF)
    rsub = torch.Tensor.__rsub__

    def rsub_bool(self, other):
        if self.dtype == torch.bool:
            assert other == 1
            return ~self
        return rsub(self, other)

    torch.Tensor.__rsub__ = rsub_bool


def case_inputs(name, all_ignored):
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2.0
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.125] = IGNORE
    if all_ignored:
        t[:] = IGNORE
    w = torch.rand(C, generator=g, dtype=torch.float64) * 2.0 + 0.1
    return x, t, w


def plant_tie(x, t, k):
    """copy the pixel of rank k (1-based, by the probability of its label) over the pixel of rank k + 4: two pixels
    then share the k-th smallest probability bit for bit"""
    rows = x.permute(0, 2, 3, 1).reshape(-1, C)
    lab = t.view(-1)
    valid = lab != IGNORE
    p = torch.softmax(rows, 1).gather(1, torch.where(valid, lab, torch.zeros_like(lab))[:, None])[:, 0]
    p = torch.where(valid, p, torch.ones_like(p))
    idx = torch.sort(p, stable=True).indices
    src, dst = int(idx[k - 1]), int(idx[k + 3])
    assert bool(valid[src]) and bool(valid[dst])
    rows = rows.clone()
    rows[dst] = rows[src]
    lab = lab.clone()
    lab[dst] = lab[src]
    return rows.view(B, H, W, C).permute(0, 3, 1, 2).contiguous(), lab.view(B, H, W)


def main():
    install_stubs()
    from utils.loss_opr import ProbOhemCrossEntropy2d
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, thresh, min_kept, reduction, weighted, all_ignored, tie in CASES:
        x, t, w = case_inputs(name, all_ignored)
        num_valid = int((t != IGNORE).sum())
        mk = num_valid + 1 if min_kept == "valid+1" else num_valid if min_kept == "valid" else int(min_kept)
        if tie:
            x, t = plant_tie(x, t, mk)
        crit = ProbOhemCrossEntropy2d(IGNORE, reduction=reduction, thresh=thresh, min_kept=mk)
        if weighted:
            crit.criterion = torch.nn.CrossEntropyLoss(reduction=reduction, weight=w, ignore_index=IGNORE)
        xr = x.clone().requires_grad_()
        loss = crit(xr, t.clone())
        loss.backward()
        kept = int((xr.grad.abs().sum(1) != 0).sum())
        print(f"{name}: valid {num_valid} min_kept {mk} thresh {thresh} kept {kept} loss {float(loss):.12g}")
        out.update({f"{name}.x": x.numpy(), f"{name}.target": t.numpy(), f"{name}.thresh": np.float64(thresh),
                    f"{name}.min_kept": np.int64(mk), f"{name}.reduction": np.array(reduction),
                    f"{name}.weight": w.numpy() if weighted else np.zeros(0), f"{name}.loss": loss.detach().numpy(),
                    f"{name}.grad": xr.grad.numpy()})
    path = os.path.join(HERE, "loss_ohem.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
