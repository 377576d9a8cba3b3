#!/usr/bin/env python3
"""The tail of the model -- 1x1 classifier, mean cross entropy and their gradients -- timed on two routes, for class
counts that are and are not multiples of 4.

    python tools/head_bench.py [--reps 30] [--warmup 5] [--out profiles/head_classes_mi355x.jsonl]
    python tools/head_bench.py --criterion weight weight_eps --out profiles/loss_options_mi355x.jsonl

Route A: the formulation up to and including the commit before the padded head: ``gemm.linear`` against the (nc, C)
weight, then ``pointwise.cross_entropy`` on the (B, nc, H, W) view, which declines rows of nc floats with nc % 4 != 0, so
the criterion itself (nn.CrossEntropyLoss) runs on the view; the classifier's gradients go to torch.mm.
Route B: what MambaDecoder.up_x4 + EncoderDecoder.forward do now: ``gemm.classifier`` (logits at a pitch of 4 ceil(nc / 4)
floats) where ``classifier_ok``, and ``pointwise.cross_entropy`` on its view.  For nc % 4 == 0 the two are the same code.

A and B alternate inside one process on one seeded (B, H, W, C) input; each repetition is one forward + backward between
two device events.  One JSON line per shape: median and spread (min, max, inter-quartile range) of each route in ms, and
each route's algorithmic bytes (what an ideal implementation of that route's passes moves; see ``route_bytes``).

``--criterion weight`` (class weights, seeded in [0.1, 2.1]) and ``weight_eps`` (the same weights and label smoothing 0.1)
time the criterion's options on the same four shapes.  Route A there is the behaviour up to the commit before the option
kernels: the head as in route B and the criterion itself, ``crit(out, label)``, on the (B, nc, H, W) view.  Route B is
``pointwise.cross_entropy`` (sigma_softmax_ce_opt_fwd / _bwd).  A third route P, the PLAIN criterion on route B's code,
alternates with them: option and plain kernels move the same algorithmic bytes, so B / P is what the options cost.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 480, 640, 96, 9), (8, 480, 640, 96, 37), (1, 720, 1280, 128, 5), (8, 480, 640, 96, 40)]
IGNORE = 255


def route_a(x, w, label, crit):
    from sigma_amd import gemm
    from sigma_amd.pointwise import cross_entropy
    out = gemm.linear(x, w.view(w.shape[0], -1)).permute(0, 3, 1, 2)
    loss = cross_entropy(crit, out, label)
    return loss if loss is not None else crit(out, label)


def route_b(x, w, label, crit):
    from sigma_amd import gemm
    from sigma_amd.pointwise import cross_entropy
    if gemm.classifier_ok(x.reshape(-1, x.shape[-1]), w):
        out = gemm.classifier(x, w).permute(0, 3, 1, 2)
    else:
        out = gemm.linear(x, w.view(w.shape[0], -1)).permute(0, 3, 1, 2)
    loss = cross_entropy(crit, out, label)
    return loss if loss is not None else crit(out, label)


def route_a_criterion(x, w, label, crit):
    """the head of route B, then the criterion itself on the view (what EncoderDecoder.forward fell through to)"""
    from sigma_amd import gemm
    if gemm.classifier_ok(x.reshape(-1, x.shape[-1]), w):
        out = gemm.classifier(x, w).permute(0, 3, 1, 2)
    else:
        out = gemm.linear(x, w.view(w.shape[0], -1)).permute(0, 3, 1, 2)
    return crit(out, label)


def criterion_bytes(M, C, nc):
    """route A of the option criteria: the GEMMs at the padded pitch, the criterion's passes on rows of nc floats (as in
    ``route_bytes``; the smoothing term's extra passes are not counted) and the copy of the gradient into padded rows"""
    ld = (nc + 3) // 4 * 4
    x, lab, z, zp = 4 * M * C, 8 * M, 4 * M * nc, 4 * M * ld
    return (x + zp) + 2 * z + 2 * z + (lab + 4 * M) + (z + lab) + 3 * z + (z + zp) + (zp + x) + (zp + x)


def route_bytes(M, C, nc):
    """algorithmic bytes of one forward + backward: every pass reads its inputs and writes its outputs once (fp32, int64
    labels, per-pixel log-sum-exp)
    kernels (B, and A for nc % 4 == 0), rows of ld = 4 ceil(nc / 4) floats:
        nt: x -> logits | loss fwd: logits, labels -> lse | loss bwd: logits, labels, lse -> dlogits |
        nn: dlogits -> dx | tn: dlogits, x -> dW
    criterion (A for nc % 4 != 0), rows of nc floats:
        nt | transposing copy to (B, nc, H, W) | log_softmax | nll (gather: labels + one logit per pixel) |
        nll backward (zero fill + scatter) | log_softmax backward (grad, output -> grad) | copy back to rows |
        mm: dlogits -> dx | mm: dlogits, x -> dW"""
    ld = (nc + 3) // 4 * 4
    x, lab, lse = 4 * M * C, 8 * M, 4 * M
    kern = (x + 4 * M * ld) + (4 * M * ld + lab + lse) + (2 * 4 * M * ld + lab + lse) + (4 * M * ld + x) + (4 * M * ld + x)
    z = 4 * M * nc
    crit = (x + z) + 2 * z + 2 * z + (lab + 4 * M) + (z + lab) + 3 * z + 2 * z + (z + x) + (z + x)
    return {"A": kern if nc % 4 == 0 else crit, "B": kern}


def spread(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "iqr_ms": round(q[2] - q[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--criterion", nargs="+", default=["plain"], choices=["plain", "weight", "weight_eps"])
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("at least 30 repetitions")
    dev = torch.device("cuda", 0)
    plain = nn.CrossEntropyLoss(reduction="mean", ignore_index=IGNORE)
    lines = []
    for B, H, W, C, nc, kind in [(*shape, kind) for kind in a.criterion for shape in SHAPES]:
        g = torch.Generator().manual_seed(1234)
        x = torch.randn(B, H, W, C, generator=g).to(dev).requires_grad_()
        w = nn.Parameter((torch.randn(nc, C, 1, 1, generator=g) / C ** 0.5).to(dev))
        label = torch.randint(0, nc, (B, H, W), generator=g)
        label[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
        label = label.to(dev)
        if kind == "plain":
            crit = plain
            routes = {"A": (route_a, crit), "B": (route_b, crit)}
        else:
            cw = (torch.rand(nc, generator=torch.Generator().manual_seed(4321)) * 2.0 + 0.1).to(dev)
            crit = nn.CrossEntropyLoss(weight=cw, reduction="mean", ignore_index=IGNORE, label_smoothing=0.1 if kind == "weight_eps" else 0.0)
            routes = {"A": (route_a_criterion, crit), "B": (route_b, crit), "P": (route_b, plain)}
        times = {k: [] for k in routes}
        losses = {}
        for i in range(a.warmup + a.reps):
            for k, (fn, c) in routes.items():
                x.grad = w.grad = None
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                loss = fn(x, w, label, c)
                loss.backward()
                t1.record()
                t1.synchronize()
                if i >= a.warmup:
                    times[k].append(t0.elapsed_time(t1))
                losses[k] = float(loss.detach())
        sa, sb = spread(times["A"]), spread(times["B"])
        line = {"shape": [B, H, W, C], "classes": nc, "reps": a.reps, "warmup": a.warmup, "A": sa, "B": sb,
                "B_over_A": round(sb["median_ms"] / sa["median_ms"], 4), "loss_A": losses["A"], "loss_B": losses["B"],
                "algorithmic_bytes": route_bytes(B * H * W, C, nc), "device": torch.cuda.get_device_name(0)}
        if kind != "plain":
            sp = spread(times["P"])
            kern = route_bytes(B * H * W, C, nc)["B"]
            line.update({"criterion": kind, "P": sp, "B_over_P": round(sb["median_ms"] / sp["median_ms"], 4), "loss_P": losses["P"],
                         "algorithmic_bytes": {"A": criterion_bytes(B * H * W, C, nc), "B": kern, "P": kern}})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del x, w, label
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
