"""GPU tests of the evaluator's device bookkeeping (csrc/segmetric.hip via sigma_amd/segmetric.py and
sigma_amd/engine/evaluator_ops.py; run with -m gpu).  Every comparison is equality: the device path does the host
path's float64 adds in the same order, numpy's arg-max rules and integer counts, so predictions, confusion matrices
and counts must be identical, not close."""
import types

import numpy as np
import pytest
import torch

from tests.model_utils import build_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def hist_info_np(n_cl, pred, gt):
    """utils/metric.py:8-15 restated: pixels with 0 <= gt < n_cl, bincount of n_cl * gt + pred"""
    k = (gt >= 0) & (gt < n_cl)
    g, p = gt[k].astype(np.int64), pred[k].astype(np.int64)
    hist = np.bincount(n_cl * g + p, minlength=n_cl ** 2).reshape(n_cl, n_cl)
    return hist, int(k.sum()), int((p == g).sum())


def sum_of_scales(rng, n_scales, shape):
    """np.zeros(float64) += float32 score, once per scale (engine/evaluator.py:437-448)"""
    acc = np.zeros(shape)
    for _ in range(n_scales):
        acc += (rng.standard_normal(shape) * rng.choice([1e-3, 1.0, 1e3])).astype(np.float32)
    return acc


def labels(rng, n_cl, shape, dtype):
    """valid classes, 255 (ignore) and values >= n_cl; int64 labels also get negative values"""
    gt = rng.randint(0, n_cl, size=shape).astype(np.int64)
    r = rng.random_sample(shape)
    gt[r < 0.1] = 255
    gt[(r >= 0.1) & (r < 0.15)] = min(n_cl + 3, 254)
    if dtype == np.int64:
        gt[(r >= 0.15) & (r < 0.2)] = -1
    return gt.astype(dtype)


def check(acc, gt, n_cl, pred_dtype=torch.int64):
    from sigma_amd import segmetric
    a = torch.from_numpy(np.ascontiguousarray(acc)).to(DEV)
    pred, (hist, labeled, correct) = segmetric.argmax_confusion(a, gt, n_cl, pred_dtype=pred_dtype)
    want = acc.argmax(0)
    got = pred.cpu().numpy()
    assert got.dtype == (np.uint8 if pred_dtype == torch.uint8 else np.int64)
    assert np.array_equal(got.astype(np.int64), want)
    rh, rl, rc = hist_info_np(n_cl, want, gt)
    assert hist.dtype == np.int64 and hist.shape == (n_cl, n_cl)
    assert np.array_equal(hist, rh) and labeled == rl and correct == rc
    return got


SIZES = [(1, 1), (7, 1001), (600, 800)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n_cl", [5, 9, 37, 40, 90, 91, 256])
def test_argmax_confusion_equals_numpy(n_cl, size):
    """float64 sums of 1-3 float32 scales, integer scores with many exact ties, +-inf / NaN at chosen pixels; uint8 and
    int64 labels with 255 and out-of-range values; int64 and uint8 predictions.  n_cl 90 / 91 straddle the LDS
    histogram budget (32 KiB), 256 is the largest n_cl."""
    if n_cl >= 90 and size == (600, 800):
        size = (61, 83)                                    # keeps the float64 scores small; the pixel loop is the same
    rng = np.random.RandomState(n_cl * 7 + size[1])
    shape = (n_cl,) + size
    gt8 = labels(rng, n_cl, size, np.uint8)
    gt64 = labels(rng, n_cl, size, np.int64)
    check(sum_of_scales(rng, 1 + n_cl % 3, shape), gt8, n_cl)
    check(sum_of_scales(rng, 3, shape), gt64, n_cl, pred_dtype=torch.uint8)
    ties = rng.randint(0, 3, size=shape).astype(np.float64)
    check(ties, gt8, n_cl)
    special = sum_of_scales(rng, 2, shape)
    flat = special.reshape(n_cl, -1)
    npix = flat.shape[1]
    picks = rng.choice(npix, size=min(npix, 64), replace=False)
    for i, p in enumerate(picks):
        kind = i % 4
        c1, c2 = rng.randint(0, n_cl, size=2)
        if kind == 0:
            flat[c1, p] = np.inf                           # first +inf wins over finite values
            flat[c2, p] = np.inf
        elif kind == 1:
            flat[c1, p] = np.nan                           # the first NaN wins over everything, +inf included
            flat[c2, p] = np.inf
        elif kind == 2:
            flat[:, p] = -np.inf                           # all -inf: class 0
        else:
            flat[c1, p] = np.nan
            flat[c2, p] = np.nan
    check(special, gt64, n_cl)
    # an image with no labeled pixel: nothing counted, the prediction still written
    pred = check(special, np.full(size, 255, np.uint8), n_cl)
    assert pred.shape == size


def test_accumulation_is_numpys_float64_sum_bitwise():
    """device acc over 3 scales == np.zeros(float64) += float32 score, bit for bit: mixed magnitudes, subnormals, -0.0
    (0.0 + -0.0 = +0.0 in the first scale, as numpy computes it), +-inf; NaN where numpy has NaN.  Both the 16-byte path
    (pixels % 4 == 0) and the scalar one."""
    from sigma_amd import segmetric
    rng = np.random.RandomState(1)
    for shape in ((40, 480, 640), (9, 7, 1001), (3, 1, 1)):
        scales = []
        for k in range(3):
            s = (rng.standard_normal(shape) * 10.0 ** rng.randint(-30, 30, size=shape)).astype(np.float32)
            flat = s.reshape(-1)
            idx = rng.choice(flat.size, size=min(flat.size, 200), replace=False)
            flat[idx[0::5]] = -0.0
            flat[idx[1::5]] = np.float32(1e-42) * rng.choice([-1, 1])
            flat[idx[2::5]] = np.inf
            flat[idx[3::5]] = -np.inf
            flat[idx[4::5]] = np.nan if k == 2 else flat[idx[4::5]]
            scales.append(s)
        want = np.zeros(shape)
        acc = torch.empty(shape, dtype=torch.float64, device=DEV)
        for k, s in enumerate(scales):
            want += s
            segmetric.accumulate_scores(acc, torch.from_numpy(s).to(DEV), first=k == 0)
        got = acc.cpu().numpy()
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got.view(np.int64)[~nan], want.view(np.int64)[~nan]), shape
        # the first scale alone: 0.0 + x
        segmetric.accumulate_scores(acc, torch.from_numpy(scales[0]).to(DEV), first=True)
        first = np.zeros(shape) + scales[0]
        assert np.array_equal(acc.cpu().numpy().view(np.int64), first.view(np.int64))


def test_hist_info_device_takes_host_and_device_inputs():
    from sigma_amd.engine import evaluator_ops as ops
    rng = np.random.RandomState(4)
    pred = rng.randint(0, 40, size=(48, 64))
    gt = labels(rng, 40, (48, 64), np.uint8)
    want = hist_info_np(40, pred, gt)
    for p, g in ((pred, gt), (torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)),
                 (pred.astype(np.int32), gt.astype(np.int16)), (pred.astype(np.uint8), torch.from_numpy(gt))):
        hist, labeled, correct = ops.hist_info_device(40, p, g)
        assert np.array_equal(hist, want[0]) and (labeled, correct) == want[1:]
    bad = pred.copy()
    bad[gt < 40] = 40                                         # a labeled pixel predicted outside the classes
    with pytest.raises(ValueError):
        ops.hist_info_device(40, bad, gt)
    with pytest.raises(TypeError):
        ops.hist_info_device(40, pred, gt.astype(np.float32))


def test_results_are_deterministic():
    """the counts are integer sums: identical from run to run, with and without torch's deterministic mode"""
    from sigma_amd import segmetric
    rng = np.random.RandomState(6)
    acc = torch.from_numpy(rng.randint(0, 4, size=(40, 480, 640)).astype(np.float64)).to(DEV)
    gt = torch.from_numpy(labels(rng, 40, (480, 640), np.uint8)).to(DEV)
    runs = []
    prev = torch.are_deterministic_algorithms_enabled()
    try:
        for det in (False, True, False, True):
            torch.use_deterministic_algorithms(det)
            pred, (hist, labeled, correct) = segmetric.argmax_confusion(acc, gt, 40)
            runs.append((pred.cpu().numpy(), hist, labeled, correct))
    finally:
        torch.use_deterministic_algorithms(prev)
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1]) and r[2:] == runs[0][2:]


class _RefEvaluator:
    """stands in for the reference's SegEvaluator: its own func_per_iteration records the prediction its
    sliding_eval_rgbX hands it (where the reference saves / shows the image)"""
    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.saved = []

    def func_per_iteration(self, data, device, config):
        self.saved.append(self.sliding_eval_rgbX(data['data'], data['modal_x'], config.eval_crop_size, config.eval_stride_rate, device))
        return {}


@pytest.mark.parametrize("crop", [(96, 128), (96, 96)], ids=["nyu-shaped-crop", "square-crop"])
def test_device_evaluation_equals_host_path(crop, monkeypatch):
    """sigma_tiny, 9 classes, eval_scale_array [0.75, 1, 1.25] with flip: sliding_eval_rgbX_device equals
    sliding_eval_rgbX element for element, and func_per_iteration returns hist_info of the host prediction.  Each
    scale's network scores are computed once and shared by both paths (the decoder's convolutions need not repeat
    bitwise from run to run), so the comparison isolates the sum, the arg-max and the counts."""
    from sigma_amd.engine import evaluator_ops as ops
    rows, cols = 96, 128
    model = build_model("sigma_tiny", 9, crop[0], crop[1]).cuda().eval()
    rng = np.random.RandomState(12)
    img = rng.randint(0, 256, size=(rows, cols, 3)).astype(np.uint8)
    mx = rng.randint(0, 256, size=(rows, cols, 3)).astype(np.uint8)
    label = labels(rng, 9, (rows, cols), np.uint8)
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    memo = {}
    scores = ops.scale_scores_device

    def shared_scores(self, img_s, *args, **kw):
        key = (img_s.shape, img_s.tobytes())
        if key not in memo:
            memo[key] = scores(self, img_s, *args, **kw)
        return memo[key]
    monkeypatch.setattr(ops, "scale_scores_device", shared_scores)
    ev = _RefEvaluator(val_func=model, norm_mean=mean, norm_std=std, is_flip=True, class_num=9, multi_scales=[0.75, 1, 1.25],
                       save_path=None, show_image=False)
    host = ops.sliding_eval_rgbX(ev, img, mx, crop, 2 / 3)
    dev = ops.sliding_eval_rgbX_device(ev, img, mx, crop, 2 / 3)
    assert len(memo) == 3
    assert dev.is_cuda and dev.dtype == torch.int64 and host.dtype == np.int64
    assert np.array_equal(dev.cpu().numpy(), host)

    config = types.SimpleNamespace(num_classes=9, eval_crop_size=crop, eval_stride_rate=2 / 3)
    data = {'data': img, 'label': label, 'modal_x': mx, 'fn': 'img0'}
    res = ops.func_per_iteration(ev, data, None, config)
    want = hist_info_np(9, host, label)
    assert set(res) == {'hist', 'labeled', 'correct'}
    assert np.array_equal(res['hist'], want[0]) and (res['labeled'], res['correct']) == want[1:]
    assert ev.saved == []                                    # nothing to save: the prediction stayed on the device
    ev.save_path = "unused"
    res2 = ops.func_per_iteration(ev, data, None, config)
    assert np.array_equal(res2['hist'], want[0]) and (res2['labeled'], res2['correct']) == want[1:]
    assert len(ev.saved) == 1 and ev.saved[0].dtype == np.int64 and np.array_equal(ev.saved[0], host)
    assert "sliding_eval_rgbX" not in ev.__dict__             # the class's method is back
