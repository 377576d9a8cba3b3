#!/usr/bin/env python3
"""Roofline table of this repository's own layout / stencil / normalisation kernels (VERDICT r2 "next" #5): each is
timed at the shapes of the sigma_small training step (batch 8: 16 encoder images, 8 decoder images) and priced against
the bytes of `read every input once + write every output once` at 6.3 TB/s (the measured copy ceiling) and 8 TB/s.

    python tools/aux_bench.py [--iters 20] [--windows 7] [--out file.jsonl] [--only dwconv,layernorm,cross_merge]

The dwconv rows carry a sha256 of out2, dx and (planes above the 48 KiB line, where the C ABI writes it) gpre from one call
through the C ABI on fixed inputs: two builds of the library (SIGMA_HIP_LIB) that print the same digests compute the same bits.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sigma_amd import ss2d_fused as sf  # noqa: E402
from sigma_amd.layernorm import LayerNorm  # noqa: E402
from sigma_amd.models.decoders.MambaDecoder import _Up2xFn  # noqa: E402
from tools.scan_bench import time_call  # noqa: E402

# (tag, images, d_inner, H, W): encoder stages 0 / 2 (2 x 8 images in one pass), decoder level at 120x160 (8 images)
STAGES = [("enc_s0", 16, 192, 120, 160), ("enc_s2", 16, 768, 30, 40), ("dec_s0", 8, 192, 120, 160)]
# encoder stages 1 and 3: dwconv rows only
DW_STAGES = [("enc_s1", 16, 384, 60, 80), ("enc_s3", 16, 1536, 15, 20)]


def _sha(t):
    return hashlib.sha256(memoryview(t.contiguous().cpu().numpy()).cast("B")).hexdigest()[:16]


def dw_case(x, w, b, orders):
    """(forward call, backward call, digests) of one dwconv problem through the C ABI on preallocated buffers, so that the
    rows time the kernels and not the allocator or the zero fill of autograd.  Digests: sha256 (first 16 hex digits) of
    out2, dx and gpre after one forward + backward; gpre only where the backward writes it (two (H + 2) x ((W + 2) | 1)
    fp32 images above 48 KiB)"""
    from sigma_amd import _capi
    lib = _capi.load()
    B, d, H, W = x.shape
    out2 = torch.empty(B, orders, d, H * W, device=x.device)
    p = _capi.DwConvParams()
    p.batch, p.channels, p.height, p.width, p.n_orders = B, d, H, W, orders
    p.x, p.weight, p.bias, p.out2 = x.data_ptr(), w.data_ptr(), b.data_ptr(), out2.data_ptr()
    g2 = torch.randn(out2.shape, generator=torch.Generator().manual_seed(1)).to(x.device)
    gpre, dx = torch.zeros_like(x), torch.empty_like(x)
    dw, db = torch.zeros(d, 9, device=x.device), torch.zeros(d, device=x.device)
    p.g2, p.gpre, p.dweight, p.dbias, p.dx = g2.data_ptr(), gpre.data_ptr(), dw.data_ptr(), db.data_ptr(), dx.data_ptr()
    keep = (out2, g2, gpre, dx, dw, db)

    def fwd(_keep=keep):
        _capi.check(lib.sigma_dwconv3x3_silu_fwd(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "dwconv fwd")

    def bwd(_keep=keep):
        _capi.check(lib.sigma_dwconv3x3_silu_bwd(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "dwconv bwd")

    fwd()
    bwd()
    torch.cuda.synchronize()
    tiled = 2 * (H + 2) * ((W + 2) | 1) * 4 > 48 * 1024
    return fwd, bwd, dict(sha_out2=_sha(out2), sha_dx=_sha(dx), sha_gpre=_sha(gpre) if tiled else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=1, help="timed windows of --iters calls per row (median and inter-quartile range)")
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="comma-separated substrings: time only the kernels whose label has one")
    a = ap.parse_args()
    only = [o for o in a.only.split(",") if o]
    dev = "cuda"
    rows = []

    def rec(kernel, tag, nbytes, fn, **extra):
        if only and not any(o in kernel for o in only):
            return
        ts = sorted(time_call(fn, a.iters) for _ in range(a.windows))      # us = the median window, iqr_us over the windows
        t = ts[len(ts) // 2]
        iqr = ts[(3 * len(ts)) // 4] - ts[len(ts) // 4]
        r = dict(kernel=kernel, shape=tag, us=round(t * 1e6, 1), iqr_us=round(iqr * 1e6, 2), MB=round(nbytes / 1e6, 1),
                 GBs=round(nbytes / t / 1e9, 1), frac_6300=round(nbytes / t / 6.3e12, 3), frac_8000=round(nbytes / t / 8e12, 3), **extra)
        rows.append(r)
        print(json.dumps(r), flush=True)

    def dw_rows(tag, x, w, b, T):
        """depthwise conv + SiLU, priced on the bytes it must move: forward 1 read + one write per order; backward one read
        per order of g2 + x, one write of dx (the gpre round trip of the two-launch backward, 2 T more, is not necessary)"""
        for orders, name in ((2, "dwconv_silu_two_orders"), (1, "dwconv_silu (one order)")):
            if only and not any(o in name for o in only):
                continue
            fwd, bwd, sha = dw_case(x, w, b, orders)
            rec(name + " fwd", tag, (1 + orders) * T, fwd, **sha)
            rec(name + " bwd", tag, (2 + orders) * T, bwd, **sha)

    for tag, B, d, H, W in DW_STAGES:
        g = torch.Generator().manual_seed(0)
        x = torch.randn(B, d, H, W, generator=g).to(dev)
        dw_rows(tag, x, (0.3 * torch.randn(d, 1, 3, 3, generator=g)).to(dev), torch.zeros(d, device=dev), B * d * H * W * 4)
        del x
    for tag, B, d, H, W in STAGES:
        L = H * W
        T = B * d * L * 4                       # bytes of one (B, d, H, W) fp32 tensor
        g = torch.Generator().manual_seed(0)
        x = torch.randn(B, d, H, W, generator=g).to(dev)
        w = (0.3 * torch.randn(d, 1, 3, 3, generator=g)).to(dev)
        b = torch.zeros(d, device=dev)
        dw_rows(tag, x, w, b, T)
        ys = torch.randn(B, 4, d, L, device=dev)
        rec("cross_merge_nhwc", tag, 5 * T, lambda: sf.cross_merge_nhwc(ys, H, W))
        dy = torch.randn(B, H, W, d, device=dev)
        rec("cross_split_nhwc", tag, 3 * T, lambda: sf.cross_split_nhwc(dy))
        du = torch.randn(B, 4 * d, L, device=dev)
        acc = torch.randn(B, 2, d, L, device=dev)
        rec("pair_sum_add", tag, 4 * T + 2 * T, lambda: sf._pair_sum_add(du, acc, B * 2, d * L))
        xz = torch.randn(B, H, W, 2 * d, device=dev, requires_grad=True)
        rec("split_xz fwd (transpose2d)", tag, 2 * T, lambda: sf.split_xz(xz))
        x1, z1 = sf.split_xz(xz)
        gx, gz = torch.randn_like(x1), torch.randn(B, H, W, d, device=dev)
        rec("split_xz bwd (transpose2d + copy)", tag, 4 * T, lambda: torch.autograd.grad((x1, z1), xz, (gx, gz), retain_graph=True))
        # LayerNorm over d (out_norm, gated) and over C = d / 2 (block norm)
        for C, gated in ((d, True), (d // 2, False)):
            ln = LayerNorm(C).to(dev)
            xin = torch.randn(B, H, W, C, device=dev, requires_grad=True)
            TC = B * L * C * 4
            if gated:
                zz = torch.randn(B, H, W, 2 * C, device=dev, requires_grad=True)
                zv = zz[..., C:]
                rec(f"layernorm gated fwd C={C}", tag, 3 * TC, lambda: ln.forward_gated(xin, zv))
                yo = ln.forward_gated(xin, zv)
                gy = torch.randn_like(yo)
                rec(f"layernorm gated bwd C={C}", tag, 5 * TC, lambda: torch.autograd.grad(yo, (xin, zz, ln.weight, ln.bias), gy, retain_graph=True))
            else:
                rec(f"layernorm fwd C={C}", tag, 2 * TC, lambda: ln(xin))
                yo = ln(xin)
                gy = torch.randn_like(yo)
                rec(f"layernorm bwd C={C}", tag, 3 * TC, lambda: torch.autograd.grad(yo, (xin, ln.weight, ln.bias), gy, retain_graph=True))
        del x, ys, dy, du, acc, xz, x1, z1
        torch.cuda.empty_cache()
    # bilinear x2 of the decoder's last two up-samplings
    for (B, H, W, C) in ((8, 120, 160, 96), (8, 240, 320, 96)):
        xin = torch.randn(B, H, W, C, device=dev, requires_grad=True)
        Tn = B * H * W * C * 4
        rec("upsample2x fwd", f"{B}x{H}x{W}x{C}", 5 * Tn, lambda: _Up2xFn.apply(xin))
        yo = _Up2xFn.apply(xin)
        gy = torch.randn_like(yo)
        rec("upsample2x bwd", f"{B}x{H}x{W}x{C}", 5 * Tn, lambda: torch.autograd.grad(yo, xin, gy, retain_graph=True))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
