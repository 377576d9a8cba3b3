"""Child process of tests/test_deterministic_gpu.py::test_whole_training_step_is_bitwise_reproducible: two training
steps of a fixture-size model (DropPath active) under torch.use_deterministic_algorithms(True), run twice from identical
state -- eagerly, then through train_step.make_graphed_step -- and compared bitwise, parameter by parameter.  Prints the
parameters whose value or gradient differ and exits 1 when any does."""
import copy
import sys

import torch


def main() -> int:
    torch.use_deterministic_algorithms(True)
    torch.utils.deterministic.fill_uninitialized_memory = False
    from sigma_amd import deterministic_enabled, train_step as ts
    from tests.model_utils import build_model, fill
    assert deterministic_enabled()
    dev = torch.device("cuda", 0)
    base = build_model("sigma_tiny", 9, 64, 96).to(dev).train()       # train mode: DropPath draws random numbers
    rgb, x, label = fill.make_inputs(2, 64, 96, 9, seed=8)
    batch = (rgb.to(dev), x.to(dev), label.to(dev))

    def run(graphed: bool):
        torch.manual_seed(1234)
        model = copy.deepcopy(base)
        opt = ts.make_optimizer(model, capturable=graphed)
        step = ts.make_graphed_step(model, opt, batch, warmup=1)[0] if graphed else ts.make_step(model, opt, batch)
        losses = [step().detach().clone() for _ in range(2)]
        torch.cuda.synchronize()
        named = [(n, p.detach().clone(), None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()]
        return losses, named

    bad = 0
    for graphed in (False, True):
        kind = "graphed" if graphed else "eager"
        (la, pa), (lb, pb) = run(graphed), run(graphed)
        if not all(torch.equal(a, b) for a, b in zip(la, lb)):
            print(f"[{kind}] loss differs: {[v.item() for v in la]} vs {[v.item() for v in lb]}")
            bad += 1
        for (n, va, ga), (_, vb, gb) in zip(pa, pb):
            if not torch.equal(va, vb):
                print(f"[{kind}] parameter differs: {n} (max |diff| {(va - vb).abs().max().item():.3e})")
                bad += 1
            if (ga is None) != (gb is None) or (ga is not None and not torch.equal(ga, gb)):
                d = float("nan") if ga is None or gb is None else (ga - gb).abs().max().item()
                print(f"[{kind}] gradient differs: {n} (max |diff| {d:.3e})")
                bad += 1
        print(f"[{kind}] {len(pa)} parameters compared, losses {[round(v.item(), 6) for v in la]}")
    if bad:
        return 1
    print("[deterministic_step_worker] done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
