"""Child process of tests/test_autograd_contract_gpu.py::test_model_autograd_contract: the fixture model tiny_64x96
(sigma_tiny, eval mode: no random depth) under torch.use_deterministic_algorithms(True) with the split-operand GEMMs
(SIGMA_GEMM=split3 and CUBLAS_WORKSPACE_CONFIG set by the parent), in the autograd configurations no other model test
runs.  Values: the fixture comparison of tests/model_utils.py at its own tolerances; everything else is exact equality.

1. baseline: every parameter trainable (the run tests/test_model_gpu.py makes); loss and gradients kept
2. freeze patterns (backbone / decode_head / the parameters in no optimizer group / everything but LayerNorm): fixture
   comparison of the trainable names, loss and trainable gradients bitwise equal to the baseline's, frozen ``.grad is
   None``, one optimizer step leaves every frozen parameter's bits alone
3. accumulation: forward + backward twice without zero_grad: fixture comparison against twice the fixture, ``.grad``
   bitwise equal to g + g
4. two micro-batches in flight (forward, forward, backward of the second, backward of the first): the sum of the
   separately computed gradients bit for bit; again into the views of train_step.flatten_grads
"""
import sys

import torch

CASE = "tiny_64x96"
TAG = "[autograd_contract_worker]"


def ok(what):
    print(f"{TAG} ok {what}", flush=True)


def grads_of(model):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}


def clear(model):
    for p in model.parameters():
        p.grad = None


def main() -> int:
    torch.use_deterministic_algorithms(True)
    from sigma_amd import deterministic_enabled, train_step
    from tests.model_utils import compare_with_reference_fixtures, fill, load_model_golden
    assert deterministic_enabled()
    meta, _ = load_model_golden(CASE)

    # 1. baseline
    model, loss0 = compare_with_reference_fixtures(CASE, "split3")
    base = grads_of(model)
    assert all(g is not None for g in base.values())
    ok("baseline")

    # 2. freeze patterns
    groups = train_step.group_weight(model, 6e-5)
    grouped = {id(p) for g in groups for p in g["params"]}
    raw = {n for n, p in model.named_parameters() if id(p) not in grouped}
    assert len(raw) == train_step.unoptimized_parameters(model, groups) > 0
    ln = {f"{mn}.{pn}" if mn else pn for mn, m in model.named_modules() if isinstance(m, torch.nn.LayerNorm)
          for pn, _ in m.named_parameters(recurse=False)}
    assert ln
    patterns = {
        "backbone": lambda n: n.startswith("backbone."),
        "decode_head": lambda n: n.startswith("decode_head."),
        "raw": lambda n: n in raw,
        "all-but-layernorm": lambda n: n not in ln,
    }
    for name, frozen in patterns.items():
        m, loss = compare_with_reference_fixtures(CASE, "split3", frozen=frozen)
        got = grads_of(m)
        n_frozen = sum(1 for n in got if frozen(n))
        assert 0 < n_frozen < len(got), (name, n_frozen)
        assert torch.equal(loss, loss0), f"{name}: loss {loss.item()!r} != baseline {loss0.item()!r}"
        bad = [n for n, g in got.items() if frozen(n) and g is not None]
        assert not bad, f"{name}: frozen parameters with a gradient: {bad[:5]}"
        bad = [n for n, g in got.items() if not frozen(n) and (g is None or not torch.equal(g, base[n]))]
        assert not bad, f"{name}: {len(bad)} trainable gradients differ from the baseline's bits: {bad[:8]}"
        before = {n: p.detach().clone() for n, p in m.named_parameters() if frozen(n)}
        opt = train_step.make_optimizer(m)
        opt.step()
        torch.cuda.synchronize()
        now = dict(m.named_parameters())
        bad = [n for n, b in before.items() if not torch.equal(now[n].detach(), b)]
        assert not bad, f"{name}: the optimizer stepped frozen parameters: {bad[:5]}"
        stepped = sum(1 for n, p in m.named_parameters() if not frozen(n) and n not in raw)
        ok(f"freeze {name}: {n_frozen} frozen, {len(got) - n_frozen} trainable ({stepped} in an optimizer group)")
        del m, opt

    # 3. accumulation
    m, loss = compare_with_reference_fixtures(CASE, "split3", grad_scale=2.0)
    assert torch.equal(loss, loss0)
    bad = [n for n, g in grads_of(m).items() if not torch.equal(g, base[n] + base[n])]
    assert not bad, f"accumulation: .grad is not g + g bit for bit: {bad[:8]}"
    ok("accumulation")

    # 4. two micro-batches in flight, on the model of 3.
    batches = []
    for seed in (1, 2):
        rgb, x, label = fill.make_inputs(meta["batch"], meta["H"], meta["W"], meta["num_classes"], seed=seed)
        batches.append((rgb.cuda(), x.cuda(), label.cuda()))
    alone = []
    for b in batches:
        clear(m)
        m(*b).backward()
        alone.append(grads_of(m))
    want = {n: alone[0][n] + alone[1][n] for n in alone[0]}

    def in_flight():
        la = m(*batches[0])
        lb = m(*batches[1])
        lb.backward()
        la.backward()
        torch.cuda.synchronize()

    clear(m)
    in_flight()
    bad = [n for n, g in grads_of(m).items() if not torch.equal(g, want[n])]
    assert not bad, f"two in flight: not the sum of the separate gradients bit for bit: {bad[:8]}"
    ok("two micro-batches in flight")

    clear(m)
    flat = train_step.flatten_grads(m)
    ptrs = {n: p.grad.data_ptr() for n, p in m.named_parameters()}
    in_flight()
    moved = [n for n, p in m.named_parameters() if p.grad.data_ptr() != ptrs[n]]
    assert not moved, f"flattened gradients: .grad left the flat buffer: {moved[:8]}"
    bad = [n for n, g in grads_of(m).items() if not torch.equal(g, want[n])]
    assert not bad, f"two in flight into the flat buffer: not the sum bit for bit: {bad[:8]}"
    cat = torch.cat([p.grad.reshape(-1) for p in m.parameters() if p.requires_grad])
    assert torch.equal(flat, cat), "the flat buffer is not the concatenation of the gradients"
    ok("two micro-batches in flight into flatten_grads")

    print(f"{TAG} done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
