"""Child process of tests/test_ohem_gpu.py::test_ohem_step_under_the_deterministic_flag: under
torch.use_deterministic_algorithms(True) one training-mode forward + backward of sigma_tiny (64x96, batch 1; 9 classes at
the padded pitch and 40 contiguous) with ProbOhemCrossEntropy2d as the criterion (class weights, a quarter of the pixels
as min_kept), run twice from identical state: nothing raises and loss and gradients are bitwise equal.  Then the class's
torch formulation on contiguous (B, 5, H, W) GPU logits, which ends in pointwise.cross_entropy_deterministic: twice the
same bits as well."""
import sys

import torch


def main() -> int:
    torch.use_deterministic_algorithms(True)
    from sigma_amd import deterministic_enabled
    from sigma_amd.pointwise import ohem_cross_entropy
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    from tests.model_utils import build_model, fill
    assert deterministic_enabled()
    dev = torch.device("cuda", 0)
    for nc in (9, 40):
        model = build_model("sigma_tiny", nc, 64, 96).to(dev).train()
        w = (torch.rand(nc, generator=torch.Generator().manual_seed(7)) * 2.0 + 0.1).to(dev)
        w[nc // 2] = 0.0
        model.criterion = ProbOhemCrossEntropy2d(255, thresh=0.7, min_kept=64 * 96 // 4, weight=w)
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
        print(f"[ohem_deterministic_worker] {nc} classes ok", flush=True)
    g = torch.Generator().manual_seed(8)
    logits = (torch.randn(2, 5, 9, 11, generator=g) * 3.0).to(dev)
    label = torch.randint(0, 5, (2, 9, 11), generator=g).to(dev)
    crit = ProbOhemCrossEntropy2d(255, thresh=0.7, min_kept=50)
    assert ohem_cross_entropy(logits, label, 255, 0.7, 50) is None
    runs = []
    for _ in range(2):
        z = logits.clone().requires_grad_()
        loss = crit(z, label)
        loss.backward()
        runs.append((loss.detach().clone(), z.grad.clone()))
    assert torch.isfinite(runs[0][0]) and torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    print("[ohem_deterministic_worker] fallback ok", flush=True)
    print("[ohem_deterministic_worker] done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
