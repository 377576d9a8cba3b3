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

    python tools/head_bench.py --ohem --out profiles/loss_ohem_mi355x.jsonl

``--ohem`` times the LOSS alone (forward + backward on given channels-last logits, no classifier) at 8 x 480 x 640 pixels
for (classes, pitch) = (40, 40) and (9, 12), min_kept = pixels / 16, thresh = 0.7, three routes alternating in one process:
a  the plain mean cross entropy on the kernels (``pointwise.cross_entropy``, the code of the commit before OHEM);
b  ``utils.loss_opr.ProbOhemCrossEntropy2d`` on the kernel route (``pointwise.ohem_cross_entropy``: one forward pass over
   the logits that also writes the per-pixel loss, the radix select, the backward on the mined labels);
c  the torch composition a user would otherwise write on the (B, nc, H, W) view: softmax, gather, sort, masked labels,
   F.cross_entropy.
b - a is what the selection costs; ``ohem_rows_bytes`` is what its rows-sized passes move, next to the logits' traffic of a.

    python tools/head_bench.py --focal --out profiles/loss_focal_mi355x.jsonl

``--focal`` times the LOSS alone in the same way, on the same two shapes, three routes alternating in one process:
a  the plain mean cross entropy on the kernels, as above;
b  ``utils.loss_opr.FocalLoss2d`` (exponent 2) on the kernel route (``pointwise.focal_cross_entropy``: the two passes of a,
   with one per-row factor);
c  the torch formulation of the class on the (B, nc, H, W) view: softmax, log_softmax, the product, nll_loss.
a and b move the same bytes, so b / a is what the per-row transcendentals cost.  Gate: b / a <= 1.10 at (40, 40), unless the
inter-quartile range of a is itself above 10 % of its median -- then the line says so and reports the spread instead.

    python tools/head_bench.py --deepsup --run 1 --out profiles/deepsup_mi355x.jsonl
    python tools/head_bench.py --deepsup --run 2 --append --out profiles/deepsup_mi355x.jsonl

``--deepsup`` times the loss term of one deep-supervision head (forward + backward on given COARSE channels-last logits, no
classifier) at the three real shapes -- batch 8, 30x40 x16, 60x80 x8, 120x160 x4, all up to 480x640 -- with 40 classes
(pitch 40) and with 9 (pitch 12), two routes alternating in one process:
fused    ``pointwise.upsampled_cross_entropy`` (csrc/deepsup.hip: the interpolation inside the loss kernels);
general  the expansion of the coarse logits to full size with two constant interpolation matrices (torch matmul) and the
         plain loss Function on the result (``pointwise.cross_entropy``), i.e. what the model does where the fused route
         declines.
``--criterion weighted | smoothed | focal | ohem`` (with --deepsup; the default is the plain criterion) times the same two
routes for a criterion with options: fused is ``pointwise.upsampled_loss``, general the criterion's own route on the expanded
logits, as the model runs it; class weights in [0.1, 2.1], smoothing 0.1 on top of them, the focal exponent 2, OHEM with
thresh 0.7 and min_kept 100000.  The lines carry ``criterion`` and ``fused_beats_general_2iqr`` (the gap above twice the
larger inter-quartile range: the rule by which the model routes a criterion to the fused kernels).
One line per (shape, classes) and one per class count for the sum over the three heads.  ``fused_beats_general``: the
difference of the medians is larger than the larger of the two inter-quartile ranges.  ``bytes``: what each route moves
algorithmically (see ``deepsup_bytes``).  A process runs at its own level (0.04 - 0.06 ms apart on these streams), which the
spread inside a process does not see: ``--run N`` tags the lines and ``--append`` adds a second process to the same file.

    python tools/head_bench.py --loss-fwd --run 1 --out profiles/loss_masked_fix_mi355x.jsonl
    SIGMA_HIP_LIB=<another build> python tools/head_bench.py --loss-fwd --run 1 --tag parent --append --out ...

``--loss-fwd`` times the FORWARD loss kernel alone (sigma_softmax_ce_fwd_ld through the C ABI, no autograd, one launch
between two device events) at 8 x 480 x 640 rows for (classes, pitch) = (68, 68) and (65, 68), the rows the walking kernel
takes (above 64 classes), and (40, 40), a register row, as the control.  One line per shape with the median and spread and
the bytes the launch moves; ``--tag`` names the build the line belongs to (the library is chosen by SIGMA_HIP_LIB), so that
two builds can alternate process by process in one session.

    python tools/head_bench.py --region --out profiles/region_loss_mi355x.jsonl

``--region`` times the region-overlap loss (csrc/region.hip) at 8 x 480 x 640 rows for (classes, pitch) = (40, 40) and
(9, 12), every launch through the C ABI between two device events, the routes alternating in one process:
region_fwd / region_bwd   sigma_region_loss_fwd (the sums and the coefficient kernel) and sigma_region_loss_bwd, Dice + CE;
ce_fwd / ce_bwd           sigma_softmax_ce_opt_fwd / _bwd on the same buffers: the yardstick, because they move the same
                          bytes -- logits and labels in, lse out; logits, labels and lse in, dlogits out;
and, forward + backward through autograd, ``RegionLoss2d`` on the kernels (function) and its torch formulation (torch).
The line reports the ratios to the cross-entropy pair; a backward above 1.25 is a finding to explain, not a failure.

    python tools/head_bench.py --distill --out profiles/distill_mi355x.jsonl

``--distill`` times the distillation loss (csrc/distill.hip) at the same rows and shapes, teacher and student at the same
pitch, T = 2, kd_all (every row in the KD term, which is what the torch composition below computes), the routes alternating in
one process:
distill_fwd / distill_bwd   sigma_distill_loss_fwd (the sums and the coefficient kernel) and sigma_distill_loss_bwd, KD + CE;
ce_fwd / ce_bwd             sigma_softmax_ce_opt_fwd / _bwd on the student's buffers: the yardstick.  The distillation launches
                            read a second row per pixel: about 2 x the bytes forward and 1.5 x backward;
and, forward + backward through autograd, ``DistillLoss2d`` on the kernels (function) and the torch composition
F.kl_div(log_softmax(x / T), softmax(t / T), "batchmean") T^2 + F.cross_entropy (torch).  The line reports each time ratio
beside its byte ratio; a time ratio above 1.3 x its byte ratio is a finding to explain, not a failure."""
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


OHEM_SHAPES = [(8, 480, 640, 40, 40), (8, 480, 640, 9, 12)]


def ohem_torch_composition(out, label, thresh, min_kept):
    """route c: ProbOhemCrossEntropy2d written with torch ops on the (B, nc, H, W) view"""
    import torch.nn.functional as F
    with torch.no_grad():
        valid = label != IGNORE
        safe = torch.where(valid, label, torch.zeros_like(label))
        p = F.softmax(out, dim=1).gather(1, safe.unsqueeze(1)).squeeze(1)
        p = torch.where(valid, p, torch.ones_like(p))
        q = torch.sort(p.reshape(-1)).values[min_kept - 1]
        keep = valid & (p <= torch.clamp(q, min=thresh))
        mined = torch.where(keep, label, torch.full_like(label, IGNORE))
    return F.cross_entropy(out, mined, ignore_index=IGNORE)


def ohem_rows_bytes(M):
    """bytes of the rows-sized passes route b adds to route a: the per-pixel loss written by the forward (4), four counting
    passes reading keys and labels (4 x 12), the final pass reading both and writing the mined labels (12 + 8)"""
    return M * (4 + 4 * 12 + 20)


def ohem_main(a, dev):
    from sigma_amd.pointwise import cross_entropy
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    plain = nn.CrossEntropyLoss(reduction="mean", ignore_index=IGNORE)
    lines = []
    for B, H, W, nc, ld in OHEM_SHAPES:
        M = B * H * W
        thresh, min_kept = 0.7, M // 16
        g = torch.Generator().manual_seed(1234)
        buf = torch.zeros(B, H, W, ld)
        buf[..., :nc] = torch.randn(B, H, W, nc, generator=g) * 3.0
        buf = buf.to(dev).requires_grad_()
        label = torch.randint(0, nc, (B, H, W), generator=g)
        label[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
        label = label.to(dev)
        ohem = ProbOhemCrossEntropy2d(IGNORE, "mean", thresh, min_kept)
        view = lambda: buf[..., :nc].permute(0, 3, 1, 2)
        routes = {"a": lambda: cross_entropy(plain, view(), label), "b": lambda: ohem(view(), label),
                  "c": lambda: ohem_torch_composition(view(), label, thresh, min_kept)}
        times = {k: [] for k in routes}
        losses = {}
        for i in range(a.warmup + a.reps):
            for k, fn in routes.items():
                buf.grad = None
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                loss = fn()
                loss.backward()
                t1.record()
                t1.synchronize()
                if i >= a.warmup:
                    times[k].append(t0.elapsed_time(t1))
                losses[k] = float(loss.detach())
        assert type(ohem(view(), label).grad_fn).__name__.startswith("OhemCEFn")
        sp = {k: spread(v) for k, v in times.items()}
        line = {"mode": "ohem", "shape": [B, H, W], "classes": nc, "ld": ld, "thresh": thresh, "min_kept": min_kept, "reps": a.reps,
                "warmup": a.warmup, "a_plain_kernels": sp["a"], "b_ohem_kernels": sp["b"], "c_ohem_torch": sp["c"],
                "b_minus_a_ms": round(sp["b"]["median_ms"] - sp["a"]["median_ms"], 4),
                "b_over_c": round(sp["b"]["median_ms"] / sp["c"]["median_ms"], 4), "loss_a": losses["a"], "loss_b": losses["b"],
                "loss_c": losses["c"], "ohem_rows_bytes": ohem_rows_bytes(M), "logits_bytes_a": 3 * 4 * M * ld,
                "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del buf, label
        torch.cuda.empty_cache()
    return lines


def focal_torch_formulation(out, label, crit):
    """route c: FocalLoss2d.forward of the reference, exponent 2, on the (B, nc, H, W) view"""
    import torch.nn.functional as F
    return crit.loss((1 - F.softmax(out, 1)) ** 2 * F.log_softmax(out, 1), label)


def focal_main(a, dev):
    from sigma_amd.pointwise import cross_entropy
    from sigma_amd.utils.loss_opr import FocalLoss2d
    plain = nn.CrossEntropyLoss(reduction="mean", ignore_index=IGNORE)
    lines = []
    for B, H, W, nc, ld in OHEM_SHAPES:
        g = torch.Generator().manual_seed(1234)
        buf = torch.zeros(B, H, W, ld)
        buf[..., :nc] = torch.randn(B, H, W, nc, generator=g) * 3.0
        buf = buf.to(dev).requires_grad_()
        label = torch.randint(0, nc, (B, H, W), generator=g)
        label[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
        label = label.to(dev)
        focal = FocalLoss2d(ignore_index=IGNORE).to(dev)
        view = lambda: buf[..., :nc].permute(0, 3, 1, 2)
        routes = {"a": lambda: cross_entropy(plain, view(), label), "b": lambda: focal(view(), label),
                  "c": lambda: focal_torch_formulation(view(), label, focal)}
        times = {k: [] for k in routes}
        losses = {}
        for i in range(a.warmup + a.reps):
            for k, fn in routes.items():
                buf.grad = None
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                loss = fn()
                loss.backward()
                t1.record()
                t1.synchronize()
                if i >= a.warmup:
                    times[k].append(t0.elapsed_time(t1))
                losses[k] = float(loss.detach())
        assert type(focal(view(), label).grad_fn).__name__.startswith("SoftmaxFocalFn")
        sp = {k: spread(v) for k, v in times.items()}
        ratio = sp["b"]["median_ms"] / sp["a"]["median_ms"]
        noisy = sp["a"]["iqr_ms"] > 0.10 * sp["a"]["median_ms"]
        line = {"mode": "focal", "shape": [B, H, W], "classes": nc, "ld": ld, "exponent": 2.0, "reps": a.reps, "warmup": a.warmup,
                "a_plain_kernels": sp["a"], "b_focal_kernels": sp["b"], "c_focal_torch": sp["c"], "b_over_a": round(ratio, 4),
                "b_over_c": round(sp["b"]["median_ms"] / sp["c"]["median_ms"], 4),
                "gate_b_over_a_1p10": ("plain route too noisy: spread reported" if noisy else "pass" if ratio <= 1.10 else "above")
                if (nc, ld) == (40, 40) else "not gated", "loss_a": losses["a"], "loss_b": losses["b"], "loss_c": losses["c"],
                "logits_bytes": 3 * 4 * B * H * W * ld, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del buf, label
        torch.cuda.empty_cache()
    return lines


DEEPSUP_SHAPES = [(8, 30, 40, 16), (8, 60, 80, 8), (8, 120, 160, 4)]
DEEPSUP_CRITERIA = ("plain", "weighted", "smoothed", "focal", "ohem")


def deepsup_bytes(B, h, w, s, ld):
    """fused: the labels (8 bytes per fine pixel) and the coarse logits read in both directions, lse (4 bytes per fine
    pixel) written once and read once, the coarse gradient written.  general: five passes over the full-size logits -- the
    expansion writes them, the loss reads them in both directions and writes their gradient, the expansion's backward reads
    it -- plus the same labels and lse and the coarse tensors at both ends."""
    P, M = B * h * s * w * s, B * h * w
    small = 2 * 4 * M * ld + 4 * M * ld
    return {"fused": 2 * 8 * P + 2 * 4 * P + small, "general": 5 * 4 * P * ld + 2 * 8 * P + 2 * 4 * P + small}


def deepsup_main(a, dev):
    from sigma_amd.models.decoders.MambaDecoder import expand_logits
    from sigma_amd.pointwise import cross_entropy, upsampled_cross_entropy, upsampled_loss
    from sigma_amd.utils.loss_opr import FocalLoss2d, ProbOhemCrossEntropy2d
    kind = a.criterion[0]
    if len(a.criterion) != 1 or kind not in DEEPSUP_CRITERIA:
        raise SystemExit(f"--deepsup takes one --criterion of {', '.join(DEEPSUP_CRITERIA)}")
    tag = {} if a.run is None else {"run": a.run}
    if kind != "plain":
        tag["criterion"] = kind
    lines = []
    for nc, ld in ((40, 40), (9, 12)):
        cw = (torch.rand(nc, generator=torch.Generator().manual_seed(7)) * 2.0 + 0.1).to(dev)
        plain = {"plain": lambda: nn.CrossEntropyLoss(reduction="mean", ignore_index=IGNORE),
                 "weighted": lambda: nn.CrossEntropyLoss(weight=cw, ignore_index=IGNORE),
                 "smoothed": lambda: nn.CrossEntropyLoss(weight=cw, ignore_index=IGNORE, label_smoothing=0.1),
                 "focal": lambda: FocalLoss2d(weight=cw, ignore_index=IGNORE).to(dev),
                 "ohem": lambda: ProbOhemCrossEntropy2d(IGNORE, thresh=0.7, min_kept=100000, weight=cw).to(dev)}[kind]()
        fused_fn = upsampled_cross_entropy if kind == "plain" else upsampled_loss
        # the general route is the model's: the criterion's own route on the expanded logits (EncoderDecoder._loss)
        general_fn = (lambda crit, out, lab: crit(out, lab)) if kind in ("focal", "ohem") else cross_entropy
        names = {"plain": ("UpsampledLossFn", "SoftmaxCEFn"), "weighted": ("UpsampledLossFn", "SoftmaxCEOptFn"),
                 "smoothed": ("UpsampledLossFn", "SoftmaxCEOptFn"), "focal": ("UpsampledLossFn", "SoftmaxFocalFn"),
                 "ohem": ("UpsampledLossFn", "OhemCEFn")}[kind]
        total = {"fused": [0.0] * a.reps, "general": [0.0] * a.reps}
        for B, h, w, s in DEEPSUP_SHAPES:
            g = torch.Generator().manual_seed(1234)
            buf = torch.zeros(B, h, w, ld)
            buf[..., :nc] = torch.randn(B, h, w, nc, generator=g) * 3.0
            buf = buf.to(dev).requires_grad_()
            label = torch.randint(0, nc, (B, h * s, w * s), generator=g)
            label[torch.rand(label.shape, generator=g) < 0.1] = IGNORE
            label = label.to(dev)
            routes = {"fused": lambda: fused_fn(plain, buf[..., :nc], s, label),
                      "general": lambda: general_fn(plain, expand_logits(buf[..., :nc], s), label)}
            times = {k: [] for k in routes}
            losses, grads = {}, {}
            for i in range(a.warmup + a.reps):
                for k, fn in routes.items():
                    buf.grad = None
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    loss = fn()
                    loss.backward()
                    t1.record()
                    t1.synchronize()
                    if i >= a.warmup:
                        times[k].append(t0.elapsed_time(t1))
                    losses[k], grads[k] = float(loss.detach()), buf.grad
            assert type(routes["fused"]().grad_fn).__name__.startswith(names[0])
            assert type(routes["general"]().grad_fn).__name__.startswith(names[1])
            for k in total:
                total[k] = [x + y for x, y in zip(total[k], times[k])]
            sp = {k: spread(v) for k, v in times.items()}
            gap = sp["general"]["median_ms"] - sp["fused"]["median_ms"]
            line = {**tag, "mode": "deepsup", "coarse": [B, h, w], "scale": s, "classes": nc, "ld": ld, "reps": a.reps, "warmup": a.warmup,
                    "fused": sp["fused"], "general": sp["general"], "general_over_fused": round(sp["general"]["median_ms"] / sp["fused"]["median_ms"], 3),
                    "fused_beats_general": bool(gap > max(sp["fused"]["iqr_ms"], sp["general"]["iqr_ms"])),
                    "loss_fused": losses["fused"], "loss_general": losses["general"],
                    "max_grad_diff": float((grads["fused"] - grads["general"]).abs().max()), "max_grad": float(grads["general"].abs().max()),
                    "bytes": deepsup_bytes(B, h, w, s, ld), "device": torch.cuda.get_device_name(0)}
            if kind != "plain":            # the routing rule of DESIGN.md 4.4: the gap above twice the larger spread
                line["fused_beats_general_2iqr"] = bool(gap > 2 * max(sp["fused"]["iqr_ms"], sp["general"]["iqr_ms"]))
            print(json.dumps(line), flush=True)
            lines.append(line)
            del buf, label, grads
            torch.cuda.empty_cache()
        sp = {k: spread(v) for k, v in total.items()}
        line = {**tag, "mode": "deepsup", "coarse": "sum of the three heads", "classes": nc, "ld": ld, "reps": a.reps, "fused": sp["fused"],
                "general": sp["general"], "general_over_fused": round(sp["general"]["median_ms"] / sp["fused"]["median_ms"], 3)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


LOSS_FWD_SHAPES = [(8, 480, 640, 68, 68), (8, 480, 640, 65, 68), (8, 480, 640, 40, 40)]


def loss_fwd_main(a, dev):
    import ctypes
    from sigma_amd import _capi
    lib = _capi.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    tag = {"build": a.tag, **({} if a.run is None else {"run": a.run})}
    lines = []
    for B, H, W, nc, ld in LOSS_FWD_SHAPES:
        rows = B * H * W
        g = torch.Generator().manual_seed(1234)
        buf = torch.zeros(rows, ld)
        buf[:, :nc] = torch.randn(rows, nc, generator=g) * 3.0
        label = torch.randint(0, nc, (rows,), generator=g)
        label[torch.rand(rows, generator=g) < 0.1] = IGNORE
        buf, label = buf.to(dev), label.to(dev)
        lse = torch.empty(rows, device=dev)
        partial = torch.empty(_capi.SIGMA_CE_BLOCKS, 2, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        times = []
        for i in range(a.warmup + a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            _capi.check(lib.sigma_softmax_ce_fwd_ld(vp(buf), vp(label), rows, nc, ld, IGNORE, vp(lse), vp(partial), st), "ce fwd ld")
            t1.record()
            t1.synchronize()
            if i >= a.warmup:
                times.append(t0.elapsed_time(t1))
        tot = partial.double().sum(0)
        line = {**tag, "mode": "loss-fwd", "rows": rows, "classes": nc, "ld": ld, "reps": a.reps, "warmup": a.warmup, "fwd": spread(times),
                "loss": float(tot[0] / tot[1]), "bytes": rows * (4 * ld + 8 + 4), "library": os.path.basename(_capi.LIB_PATH),
                "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del buf, label, lse
        torch.cuda.empty_cache()
    return lines


def region_main(a, dev):
    import ctypes
    from sigma_amd import _capi, _capi_region
    from sigma_amd.utils.loss_opr import RegionLoss2d
    lib = _capi_region.load()
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []
    for B, H, W, nc, ld in OHEM_SHAPES:
        rows = B * H * W
        g = torch.Generator().manual_seed(1234)
        buf = torch.zeros(rows, ld)
        buf[:, :nc] = torch.randn(rows, nc, generator=g) * 3.0
        label = torch.randint(0, nc, (rows,), generator=g)
        label[torch.rand(rows, generator=g) < 0.1] = IGNORE
        buf, label = buf.to(dev), label.to(dev)
        f32 = dict(device=dev, dtype=torch.float32)
        lse, dl, scale = torch.empty(rows, **f32), torch.empty(rows, ld, **f32), torch.ones(1, **f32)
        out, coef = torch.empty(3 + 3 * nc, **f32), torch.empty(2 * nc + 1, **f32)
        r = _capi_region.RegionParams()
        r.rows, r.classes, r.ld, r.ignore_index = rows, nc, ld, IGNORE
        r.alpha, r.beta, r.smooth, r.region_weight, r.ce_weight = 0.5, 0.5, 1.0, 1.0, 1.0
        r.logits, r.labels, r.lse, r.coef = buf.data_ptr(), label.data_ptr(), lse.data_ptr(), coef.data_ptr()
        ws = torch.empty(int(lib.sigma_region_loss_workspace_bytes(ctypes.byref(r))), device=dev, dtype=torch.uint8)
        r.workspace, r.workspace_bytes = ws.data_ptr(), ws.numel()
        r.loss, r.terms, r.sums = out.data_ptr(), out[1:].data_ptr(), out[3:].data_ptr()
        r.scale, r.dlogits = scale.data_ptr(), dl.data_ptr()
        partial = torch.empty(_capi.SIGMA_CE_BLOCKS, 2, **f32)
        c = _capi.CeOptParams()
        c.rows, c.classes, c.ld, c.ignore_index = rows, nc, ld, IGNORE
        c.logits, c.labels, c.lse, c.partial = buf.data_ptr(), label.data_ptr(), lse.data_ptr(), partial.data_ptr()
        c.scale, c.dlogits = scale.data_ptr(), dl.data_ptr()
        launches = {"region_fwd": lambda: lib.sigma_region_loss_fwd(ctypes.byref(r), st()),
                    "ce_fwd": lambda: lib.sigma_softmax_ce_opt_fwd(ctypes.byref(c), st()),
                    "region_bwd": lambda: lib.sigma_region_loss_bwd(ctypes.byref(r), st()),
                    "ce_bwd": lambda: lib.sigma_softmax_ce_opt_bwd(ctypes.byref(c), st())}
        crit = RegionLoss2d("dice", ignore_index=IGNORE, smooth=1.0, ce_weight=1.0)
        leaf = buf.view(B, H, W, ld).requires_grad_()
        view = lambda: leaf[..., :nc].permute(0, 3, 1, 2)
        label3 = label.view(B, H, W)
        routes = {"function": lambda: crit(view(), label3), "torch": lambda: crit.torch_formulation(view(), label3)}
        times = {k: [] for k in (*launches, *routes)}
        losses = {}
        for i in range(a.warmup + a.reps):
            for k in times:
                leaf.grad = None
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                if k in launches:
                    _capi.check(launches[k](), k)
                else:
                    loss = routes[k]()
                    loss.backward()
                    losses[k] = loss.detach()
                t1.record()
                t1.synchronize()
                if i >= a.warmup:
                    times[k].append(t0.elapsed_time(t1))
        assert crit.last_terms is not None
        sp = {k: spread(v) for k, v in times.items()}
        med = lambda k: sp[k]["median_ms"]
        line = {"mode": "region", "rows": rows, "classes": nc, "ld": ld, "kind": "dice", "ce_weight": 1.0, "reps": a.reps, "warmup": a.warmup,
                **sp, "fwd_over_ce": round(med("region_fwd") / med("ce_fwd"), 4), "bwd_over_ce": round(med("region_bwd") / med("ce_bwd"), 4),
                "bwd_above_1p25": med("region_bwd") > 1.25 * med("ce_bwd"),
                "function_over_torch": round(med("function") / med("torch"), 4),
                "fwd_bytes": rows * (4 * ld + 8 + 4), "bwd_bytes": rows * (8 * ld + 8 + 4),
                "loss_function": float(losses["function"]), "loss_torch": float(losses["torch"]), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del buf, label, lse, dl, leaf, ws
        torch.cuda.empty_cache()
    return lines


def distill_main(a, dev):
    import ctypes
    import torch.nn.functional as F
    from sigma_amd import _capi, _capi_distill
    from sigma_amd.utils.loss_opr import DistillLoss2d
    lib = _capi_distill.load()
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    T, kw, cw = 2.0, 1.0, 1.0
    lines = []
    for B, H, W, nc, ld in OHEM_SHAPES:
        rows = B * H * W
        g = torch.Generator().manual_seed(1234)
        buf, tbuf = torch.zeros(rows, ld), torch.zeros(rows, ld)
        buf[:, :nc] = torch.randn(rows, nc, generator=g) * 3.0
        tbuf[:, :nc] = 0.7 * buf[:, :nc] + torch.randn(rows, nc, generator=g) * 2.0
        label = torch.randint(0, nc, (rows,), generator=g)
        label[torch.rand(rows, generator=g) < 0.1] = IGNORE
        buf, tbuf, label = buf.to(dev), tbuf.to(dev), label.to(dev)
        f32 = dict(device=dev, dtype=torch.float32)
        lse, lse3, dl, scale = torch.empty(rows, **f32), torch.empty(rows, 3, **f32), torch.empty(rows, ld, **f32), torch.ones(1, **f32)
        out, coef = torch.empty(3, **f32), torch.empty(2, **f32)
        d = _capi_distill.DistillParams()
        d.rows, d.classes, d.ld, d.ld_t, d.kd_all, d.ignore_index = rows, nc, ld, ld, 1, IGNORE
        d.temperature, d.kd_weight, d.ce_weight = T, kw, cw
        d.logits, d.teacher, d.labels, d.lse, d.coef = buf.data_ptr(), tbuf.data_ptr(), label.data_ptr(), lse3.data_ptr(), coef.data_ptr()
        ws = torch.empty(int(lib.sigma_distill_loss_workspace_bytes(ctypes.byref(d))), device=dev, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        d.loss, d.terms = out.data_ptr(), out[1:].data_ptr()
        d.scale, d.dlogits = scale.data_ptr(), dl.data_ptr()
        partial = torch.empty(_capi.SIGMA_CE_BLOCKS, 2, **f32)
        c = _capi.CeOptParams()
        c.rows, c.classes, c.ld, c.ignore_index = rows, nc, ld, IGNORE
        c.logits, c.labels, c.lse, c.partial = buf.data_ptr(), label.data_ptr(), lse.data_ptr(), partial.data_ptr()
        c.scale, c.dlogits = scale.data_ptr(), dl.data_ptr()
        launches = {"distill_fwd": lambda: lib.sigma_distill_loss_fwd(ctypes.byref(d), st()),
                    "ce_fwd": lambda: lib.sigma_softmax_ce_opt_fwd(ctypes.byref(c), st()),
                    "distill_bwd": lambda: lib.sigma_distill_loss_bwd(ctypes.byref(d), st()),
                    "ce_bwd": lambda: lib.sigma_softmax_ce_opt_bwd(ctypes.byref(c), st())}
        crit = DistillLoss2d(T, kw, cw, ignore_index=IGNORE, kd_all=True)
        leaf = buf.view(B, H, W, ld).requires_grad_()
        view = lambda: leaf[..., :nc].permute(0, 3, 1, 2)
        tview = tbuf.view(B, H, W, ld)[..., :nc].permute(0, 3, 1, 2)
        label3 = label.view(B, H, W)

        def composition():
            x2, t2 = leaf[..., :nc].reshape(-1, nc), tbuf.view(B, H, W, ld)[..., :nc].reshape(-1, nc)
            kd = F.kl_div(F.log_softmax(x2 / T, dim=1), F.softmax(t2 / T, dim=1), reduction="batchmean") * (T * T)
            return kw * kd + cw * F.cross_entropy(x2, label, ignore_index=IGNORE)

        routes = {"function": lambda: crit(view(), label3, tview), "torch": composition}
        times = {k: [] for k in (*launches, *routes)}
        losses = {}
        for i in range(a.warmup + a.reps):
            for k in times:
                leaf.grad = None
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                if k in launches:
                    _capi.check(launches[k](), k)
                else:
                    loss = routes[k]()
                    loss.backward()
                    losses[k] = loss.detach()
                t1.record()
                t1.synchronize()
                if i >= a.warmup:
                    times[k].append(t0.elapsed_time(t1))
        assert crit.last_terms is not None
        sp = {k: spread(v) for k, v in times.items()}
        med = lambda k: sp[k]["median_ms"]
        by = dict(distill_fwd=rows * (8 * ld + 8 + 12), ce_fwd=rows * (4 * ld + 8 + 4), distill_bwd=rows * (12 * ld + 8 + 12),
                  ce_bwd=rows * (8 * ld + 8 + 4))
        fwd_t, bwd_t = med("distill_fwd") / med("ce_fwd"), med("distill_bwd") / med("ce_bwd")
        fwd_b, bwd_b = by["distill_fwd"] / by["ce_fwd"], by["distill_bwd"] / by["ce_bwd"]
        line = {"mode": "distill", "rows": rows, "classes": nc, "ld": ld, "ld_t": ld, "temperature": T, "kd_all": True, "ce_weight": cw,
                "reps": a.reps, "warmup": a.warmup, **sp,
                "fwd_over_ce": round(fwd_t, 4), "fwd_bytes_over_ce": round(fwd_b, 4), "fwd_above_1p3_bytes": fwd_t > 1.3 * fwd_b,
                "bwd_over_ce": round(bwd_t, 4), "bwd_bytes_over_ce": round(bwd_b, 4), "bwd_above_1p3_bytes": bwd_t > 1.3 * bwd_b,
                "torch_over_function": round(med("torch") / med("function"), 4), **{k + "_bytes": v for k, v in by.items()},
                "fwd_tb_per_s": round(by["distill_fwd"] / med("distill_fwd") / 1e9, 3),
                "bwd_tb_per_s": round(by["distill_bwd"] / med("distill_bwd") / 1e9, 3),
                "loss_function": float(losses["function"]), "loss_torch": float(losses["torch"]), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del buf, tbuf, label, lse, lse3, dl, leaf, ws
        torch.cuda.empty_cache()
    return lines


def spread(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "iqr_ms": round(q[2] - q[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--criterion", nargs="+", default=["plain"], choices=["plain", "weight", "weight_eps", "weighted", "smoothed", "focal", "ohem"],
                    help="plain / weight / weight_eps: the head shapes; --deepsup: one of plain, weighted, smoothed, focal, ohem")
    ap.add_argument("--ohem", action="store_true", help="time the OHEM loss against the plain loss and a torch composition")
    ap.add_argument("--focal", action="store_true", help="time the focal loss against the plain loss and the torch formulation")
    ap.add_argument("--deepsup", action="store_true", help="time the fused upsample + loss of a deep-supervision head against the expansion")
    ap.add_argument("--loss-fwd", action="store_true", help="time the forward loss kernel alone at 68, 65 and 40 classes")
    ap.add_argument("--region", action="store_true", help="time the region-overlap loss against the cross-entropy kernels and its torch formulation")
    ap.add_argument("--distill", action="store_true", help="time the distillation loss against the cross-entropy kernels and the torch composition")
    ap.add_argument("--tag", default="tree", help="--loss-fwd: the name of the build the lines belong to")
    ap.add_argument("--run", type=int, default=None, help="--deepsup / --loss-fwd: tag every line with this run number (one process per run)")
    ap.add_argument("--append", action="store_true", help="--deepsup / --loss-fwd: add the lines to --out instead of replacing it")
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("at least 30 repetitions")
    dev = torch.device("cuda", 0)
    if a.ohem or a.focal or a.deepsup or a.loss_fwd or a.region or a.distill:
        lines = distill_main(a, dev) if a.distill else region_main(a, dev) if a.region else ohem_main(a, dev) if a.ohem else focal_main(a, dev) if a.focal else deepsup_main(a, dev) if a.deepsup else loss_fwd_main(a, dev)
        if a.out:
            with open(a.out, "a" if (a.deepsup or a.loss_fwd) and a.append else "w") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")
        return
    if not set(a.criterion) <= {"plain", "weight", "weight_eps"}:
        ap.error("weighted, smoothed, focal and ohem are criteria of --deepsup")
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
