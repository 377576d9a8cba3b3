"""The trajectory checker of tests/train_trajectory.py is sharp: on a small CPU model (eager steps, the optimizer and
groups of sigma_amd.train_step) two identical runs report nothing, and each of four wrong runs -- the mistakes a captured
step can make without raising -- is reported at the step where it happens, with the kinds and names it touches and no
others.  Also here: the CPU-checkable part of resuming a captured step from a checkpoint (train_step._tensor_lrs)."""
import io

import pytest
import torch
import torch.nn as nn

from sigma_amd import train_step as ts
from tests import train_trajectory as tt
from tests.test_ddp_gloo import TinySeg

STEPS, K = 4, 2                                      # the wrong runs go wrong at step K
RATES = [1.5e-3, 3e-3, 6e-3, 4.2e-3]                 # neighbours differ by at least 1.4x
DECAY = {"stem.weight", "head.weight"}
GROUPED = DECAY | {"stem.bias", "head.bias", "norm.weight", "norm.bias"}


def _batch(t):
    g = torch.Generator().manual_seed(200 + t)
    return (torch.randn(2, 3, 16, 16, generator=g), torch.randn(2, 3, 16, 16, generator=g),
            torch.randint(0, 5, (2, 16, 16), generator=g))


def _run(skip_step_at=None, stale_rate_at=None, no_decay_from=None, zero_update_at=None, touch_raw_at=None):
    torch.manual_seed(0)
    model = TinySeg()
    opt = ts.make_optimizer(model, lr=6e-3)
    state = dict(t=0)

    def before(t):
        state["t"] = t
        if t != stale_rate_at:
            ts.set_lr(opt, RATES[t])
        if t == no_decay_from:
            opt.param_groups[0]["weight_decay"] = 0.0

    def step():
        t = state["t"]
        opt.zero_grad(set_to_none=True)
        loss = model(*_batch(t))
        loss.backward()
        kept = model.head.weight.detach().clone()
        if t != skip_step_at:
            opt.step()
        if t == zero_update_at:
            with torch.no_grad():
                model.head.weight.copy_(kept)
        if t == touch_raw_at:
            with torch.no_grad():
                model.scale.mul_(1.0 + 2.0 ** -20)
        return loss

    return tt.record(model, opt, step, STEPS, before)


@pytest.fixture(scope="module")
def good():
    return _run()


def _at(entries, t):
    return {(kind, name) for s, kind, name in entries if s == t}


def test_identical_runs_report_nothing_and_the_correct_run_moves(good):
    assert tt.compare(good, _run()) == []
    assert tt.movement_violations(good) == []
    assert good.grouped == GROUPED
    assert ts.unoptimized_parameters(good.model, good.opt.param_groups) == 1          # TinySeg.scale
    assert set(good.steps[0]["param"]) - good.grouped == {"scale"}
    assert bool(good.steps[0]["grad"]["scale"].any())                               # it has a gradient and still never moves
    assert [float(r["lr"]["group1"]) for r in good.steps] == [float(torch.tensor(v)) for v in RATES]
    assert [float(r["step"]["head.bias"]) for r in good.steps] == [1.0, 2.0, 3.0, 4.0]


def test_a_skipped_optimizer_step_is_reported(good):
    bad = _run(skip_step_at=K)
    diff = tt.compare(good, bad)
    assert min(t for t, _, _ in diff) == K
    want = {(kind, n) for kind in ("param", "exp_avg", "exp_avg_sq", "step") for n in GROUPED}
    assert _at(diff, K) == want, tt.describe(diff)               # same state going in: loss and gradients still agree
    assert ("loss", "loss") in _at(diff, K + 1)
    assert _at(tt.movement_violations(bad), K) == {("unmoved", n) for n in GROUPED}
    assert all(t == K for t, _, _ in tt.movement_violations(bad))


def test_a_rate_that_was_not_applied_is_reported(good):
    bad = _run(stale_rate_at=K)
    diff = tt.compare(good, bad)
    assert min(t for t, _, _ in diff) == K
    want = {("param", n) for n in GROUPED} | {("lr", "group0"), ("lr", "group1")}
    assert _at(diff, K) == want, tt.describe(diff)               # the moments do not depend on the rate
    assert tt.movement_violations(bad) == []                     # it did move: only the comparison can see this one
    # a stale rate that the recorded lr cannot show (the tensor was written, the kernel read another): parameters alone
    assert {n for kind, n in _at(tt.compare(good, bad, kinds=("param",)), K)} == GROUPED


def test_dropped_weight_decay_is_reported(good):
    bad = _run(no_decay_from=K)
    diff = tt.compare(good, bad)
    assert min(t for t, _, _ in diff) == K
    assert _at(diff, K) == {("param", n) for n in DECAY}, tt.describe(diff)
    assert tt.movement_violations(bad) == []


def test_one_zeroed_update_is_reported(good):
    bad = _run(zero_update_at=K)
    diff = tt.compare(good, bad)
    assert min(t for t, _, _ in diff) == K
    assert _at(diff, K) == {("param", "head.weight")}, tt.describe(diff)
    assert tt.movement_violations(bad) == [(K, "unmoved", "head.weight")]


def test_a_parameter_outside_every_group_must_not_move(good):
    bad = _run(touch_raw_at=K)
    assert tt.movement_violations(bad) == [(t, "moved-ungrouped", "scale") for t in range(K, STEPS)]
    assert _at(tt.compare(good, bad), K) == {("param", "scale")}


def test_a_missing_gradient_or_state_entry_is_a_difference(good):
    other = _run()
    other.steps[1]["grad"]["norm.bias"] = None
    del other.steps[3]["exp_avg"]["stem.bias"]
    assert tt.compare(good, other) == [(1, "grad", "norm.bias"), (3, "exp_avg", "stem.bias")]


def test_a_checkpointed_tensor_rate_arrives_on_the_cpu_and_is_moved_to_the_groups_device():
    """Resume: ``Optimizer.load_state_dict`` takes ``param_groups[i]['lr']`` as the checkpoint holds it -- for
    ``torch.load(map_location="cpu")`` a CPU tensor, whatever device the parameters are on -- and ``_tensor_lrs`` moves a
    tensor rate that is not on its group's device there (shown with parameters on the meta device: no GPU here; values on
    the GPU: tests/graph_step_worker.py graph-resume).  A rate already in place is kept as the object it is."""
    model = TinySeg()
    opt = ts.make_optimizer(model, lr=1e-2)
    for g in opt.param_groups:
        g["lr"] = torch.tensor(2.5e-3)                # what make_optimizer(capturable=True) builds on the GPU
    model(*_batch(0)).backward()
    opt.step()
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    fresh = ts.make_optimizer(TinySeg(), lr=1e-2)
    fresh.load_state_dict(torch.load(buf, map_location="cpu"))
    rates = [g["lr"] for g in fresh.param_groups]
    assert all(torch.is_tensor(v) and v.device.type == "cpu" and float(v) == float(torch.tensor(2.5e-3)) for v in rates)
    ts._tensor_lrs(fresh)                             # CPU parameters, CPU rates: nothing to move
    assert all(g["lr"] is v for g, v in zip(fresh.param_groups, rates))
    ts.set_lr(fresh, 5e-3)
    assert all(g["lr"] is v and float(v) == float(torch.tensor(5e-3)) for g, v in zip(fresh.param_groups, rates))
    # parameters elsewhere than the rate: the rate follows them
    lin = nn.Linear(4, 4, device="meta")
    moved = torch.optim.SGD([dict(params=[lin.weight], lr=torch.tensor(2.5e-3)), dict(params=[lin.bias], lr=torch.tensor(1e-3))], lr=1e-3)
    ts._tensor_lrs(moved)
    assert all(g["lr"].device.type == "meta" and g["lr"].dtype == torch.float32 and g["lr"].shape == () for g in moved.param_groups)
