#!/usr/bin/env python3
"""Forward-only (eval, no_grad) throughput of the HIP path -- BASELINE.json configs[1]:
    python tools/eval_bench.py [--backbone sigma_tiny] [--batch 2] [--height 480 --width 640] [--iters 10]

The evaluation loop per image at NYU settings (--eval-loop host|device; sigma_small, 40 classes, synthetic 480 x 640
uint8 pairs, eval_scale_array [0.75, 1, 1.25], flip, crop 480 x 640, stride 2/3), one path per process:
    python tools/eval_bench.py --eval-loop host   [--images 6]   # sliding_eval_rgbX + hist_info on the host
    python tools/eval_bench.py --eval-loop device [--images 6]   # func_per_iteration: sum, arg-max, counts on the device
Prints ms/image of the whole loop and of the bookkeeping alone (the same per-scale device scores, precomputed, taken
through the path's sum / arg-max / confusion)."""
import argparse, json, os, sys, time, types
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="sigma_tiny")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--eval-loop", choices=("host", "device"), default=None)
    ap.add_argument("--images", type=int, default=6)
    a = ap.parse_args()
    if a.eval_loop:
        return eval_loop(a)
    from sigma_amd.models.builder import EncoderDecoder
    from sigma_amd.tuning import enable_tuned_gemms
    enable_tuned_gemms()
    cfg = types.SimpleNamespace(backbone=a.backbone, decoder="MambaDecoder", num_classes=a.classes, image_height=a.height,
                                image_width=a.width, pretrained_model=None, bn_eps=1e-3, bn_momentum=0.1)
    cwd = os.getcwd(); os.chdir("/tmp")
    try:
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            model = EncoderDecoder(cfg).cuda().eval()
    finally:
        os.chdir(cwd)
    g = torch.Generator().manual_seed(0)
    rgb = torch.randn(a.batch, 3, a.height, a.width, generator=g).cuda()
    x = torch.randn(a.batch, 3, a.height, a.width, generator=g).cuda()
    with torch.no_grad():
        for _ in range(3):
            model(rgb, x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            model(rgb, x)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.iters
    print(json.dumps(dict(metric=f"images/sec fwd only {a.backbone} {a.height}x{a.width}", value=round(a.batch / dt, 2),
                          ms_per_forward=round(dt * 1e3, 2), batch=a.batch, dtype="f32")))


def hist_info_np(n_cl, pred, gt):
    """utils/metric.py:8-15 restated (boolean mask, bincount over the pixels on the host)"""
    k = (gt >= 0) & (gt < n_cl)
    return (np.bincount(n_cl * gt[k].astype(int) + pred[k].astype(int), minlength=n_cl ** 2).reshape(n_cl, n_cl),
            np.sum(k), np.sum(pred[k] == gt[k]))


def eval_loop(a):
    from sigma_amd.engine import evaluator_ops as ops
    from sigma_amd.models.builder import EncoderDecoder
    from sigma_amd.tuning import enable_tuned_gemms
    enable_tuned_gemms()
    H, W, n_cl, crop, scales = 480, 640, 40, (480, 640), [0.75, 1, 1.25]
    cfg = types.SimpleNamespace(backbone="sigma_small", decoder="MambaDecoder", num_classes=n_cl, image_height=H,
                                image_width=W, pretrained_model=None, bn_eps=1e-3, bn_momentum=0.1)
    cwd = os.getcwd(); os.chdir("/tmp")
    try:
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            model = EncoderDecoder(cfg).cuda().eval()
    finally:
        os.chdir(cwd)
    ev = types.SimpleNamespace(val_func=model, norm_mean=np.array([0.485, 0.456, 0.406]), norm_std=np.array([0.229, 0.224, 0.225]),
                               is_flip=True, class_num=n_cl, multi_scales=scales, save_path=None, show_image=False)
    config = types.SimpleNamespace(num_classes=n_cl, eval_crop_size=crop, eval_stride_rate=2 / 3)
    rng = np.random.RandomState(0)
    images = []
    for i in range(a.images + 1):                       # image 0 warms up
        label = rng.randint(0, n_cl, size=(H, W)).astype(np.uint8)
        label[rng.random_sample((H, W)) < 0.1] = 255
        images.append({'data': rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8), 'label': label,
                       'modal_x': rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8), 'fn': f"img{i}"})

    def per_image(d):
        if a.eval_loop == "host":
            pred = ops.sliding_eval_rgbX(ev, d['data'], d['modal_x'], crop, 2 / 3)
            hist, labeled, correct = hist_info_np(n_cl, pred, d['label'])
            return int(labeled)
        return ops.func_per_iteration(ev, d, None, config)['labeled']

    dev = torch.device("cuda", 0)
    with torch.no_grad():
        per_image(images[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for d in images[1:]:
            per_image(d)
        torch.cuda.synchronize()
        loop_ms = (time.perf_counter() - t0) / a.images * 1e3
        # the bookkeeping alone: the three per-scale (C, H, W) device scores of one image, precomputed
        d = images[1]
        scores = [ops.scale_scores_device(ev, ops.resize_like_cv2(d['data'], s, False, dev), ops.resize_like_cv2(d['modal_x'], s, False, dev),
                                          (H, W), crop, 2 / 3) for s in scales]
        from sigma_amd import segmetric

        def bookkeeping():
            if a.eval_loop == "host":
                processed = np.zeros((H, W, n_cl))
                for sc in scores:
                    processed += sc.permute(1, 2, 0).contiguous().cpu().numpy()
                return hist_info_np(n_cl, processed.argmax(2), d['label'])
            acc = torch.empty((n_cl, H, W), dtype=torch.float64, device=dev)
            for k, sc in enumerate(scores):
                segmetric.accumulate_scores(acc, sc, k == 0)
            return segmetric.argmax_confusion(acc, d['label'], n_cl, want_pred=False)[1]
        bookkeeping()
        torch.cuda.synchronize()
        reps = 10
        t0 = time.perf_counter()
        for _ in range(reps):
            bookkeeping()
        torch.cuda.synchronize()
        book_ms = (time.perf_counter() - t0) / reps * 1e3
    print(json.dumps(dict(metric=f"eval loop ms/image ({a.eval_loop} bookkeeping) sigma_small {H}x{W} {n_cl} classes, scales {scales}, flip",
                          path=a.eval_loop, ms_per_image=round(loop_ms, 2), bookkeeping_ms_per_image=round(book_ms, 2),
                          images=a.images)))


if __name__ == "__main__":
    main()
