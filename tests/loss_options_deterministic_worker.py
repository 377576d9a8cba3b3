"""Child process of tests/test_loss_options_gpu.py::test_weighted_step_under_the_deterministic_flag: one training-mode
forward + backward of sigma_tiny (64x96, batch 1; 9 classes at the padded pitch and 40 contiguous) with a weighted,
label-smoothed criterion under torch.use_deterministic_algorithms(True), run twice from identical state: the step runs
(torch's nll_loss2d would raise) and loss and gradients are bitwise equal."""
import sys

import torch
import torch.nn as nn


def main() -> int:
    torch.use_deterministic_algorithms(True)
    from sigma_amd import deterministic_enabled
    from tests.model_utils import build_model, fill
    assert deterministic_enabled()
    dev = torch.device("cuda", 0)
    for nc in (9, 40):
        model = build_model("sigma_tiny", nc, 64, 96).to(dev).train()
        w = (torch.rand(nc, generator=torch.Generator().manual_seed(7)) * 2.0 + 0.1).to(dev)
        w[nc // 2] = 0.0
        model.criterion = nn.CrossEntropyLoss(weight=w, ignore_index=255, label_smoothing=0.1)
        rgb, x, label = (t.to(dev) for t in fill.make_inputs(1, 64, 96, nc, seed=5))
        runs = []
        for _ in range(2):
            torch.manual_seed(1234)                       # DropPath draws random numbers
            model.zero_grad(set_to_none=True)
            loss = model(rgb, x, label)
            loss.backward()
            torch.cuda.synchronize()
            runs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}))
        (l0, g0), (l1, g1) = runs
        assert torch.isfinite(l0) and torch.equal(l0, l1), (l0, l1)
        differ = [n for n in g0 if not torch.equal(g0[n], g1[n])]
        assert not differ, differ
        assert all(bool(torch.isfinite(g).all()) for g in g0.values())
        print(f"[loss_options_deterministic_worker] {nc} classes ok", flush=True)
    print("[loss_options_deterministic_worker] done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
