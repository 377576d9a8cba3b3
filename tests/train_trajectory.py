"""Trajectories of training steps, compared bit for bit (tests/test_train_trajectory_cpu.py, tests/graph_step_worker.py).

A trajectory holds, after every step: the loss, every named parameter and buffer (BatchNorm's running statistics are
written by a training-mode forward), every ``.grad``, and the optimizer's state (``exp_avg``, ``exp_avg_sq``, ``step`` per
parameter, ``lr`` per group).  ``compare(a, b)`` lists what is not
``torch.equal``; ``movement_violations(t)`` checks, without a numeric threshold, that the optimizer did step what it owns
and nothing else:

  * at every step, every parameter tensor that is in an optimizer group and whose gradient is not identically zero
    differs from its value one step earlier in at least one element;
  * every parameter in no group (by default the raw Mamba parameters, train_step.unoptimized_parameters counts them)
    is bitwise what it was before the first step, at every step.

A comparison of two trajectories alone cannot see an optimizer that never ran on BOTH sides; the movement condition on
one of them can."""
from typing import Callable, Dict, List, Optional, Tuple

import torch

# per step, in the order a difference is reported: what the step computes first comes first
KINDS = ("loss", "buffer", "grad", "lr", "step", "exp_avg", "exp_avg_sq", "param")
Entry = Tuple[int, str, str]


def snapshot(model: torch.nn.Module, opt, loss: Optional[torch.Tensor] = None) -> Dict[str, Dict[str, Optional[torch.Tensor]]]:
    """{kind: {name: copy of the tensor, or None where there is none}} of the state as it stands"""
    names = {id(p): n for n, p in model.named_parameters()}
    rec = {k: {} for k in KINDS}
    if loss is not None:
        rec["loss"]["loss"] = loss.detach().clone()
    for n, p in model.named_parameters():
        rec["param"][n] = p.detach().clone()
        rec["grad"][n] = None if p.grad is None else p.grad.detach().clone()
    for n, b in model.named_buffers():
        rec["buffer"][n] = b.detach().clone()
    for i, g in enumerate(opt.param_groups):
        # a float rate and a tensor rate of the same value are the same rate: both are recorded as the fp32 the kernel reads
        rec["lr"][f"group{i}"] = torch.tensor(float(g["lr"]), dtype=torch.float32)
        for p in g["params"]:
            st = opt.state.get(p, {})
            for k in ("step", "exp_avg", "exp_avg_sq"):
                v = st.get(k)
                rec[k][names[id(p)]] = v.detach().clone() if torch.is_tensor(v) else None if v is None else torch.tensor(float(v))
    return rec


class Trajectory:
    """``start``: the snapshot before the first recorded step; ``steps``: one snapshot after each; ``grouped``: the names
    of the parameters some optimizer group owns"""

    def __init__(self, model: torch.nn.Module, opt):
        self.model, self.opt = model, opt
        names = {id(p): n for n, p in model.named_parameters()}
        self.grouped = {names[id(p)] for g in opt.param_groups for p in g["params"]}
        self.start = snapshot(model, opt)
        self.steps: List[dict] = []

    def add(self, loss: torch.Tensor) -> None:
        self.steps.append(snapshot(self.model, self.opt, loss))

    def rebind(self, model: torch.nn.Module, opt) -> None:
        """go on recording from another model / optimizer pair holding the same run (a resume from a checkpoint)"""
        names = {id(p): n for n, p in model.named_parameters()}
        grouped = {names[id(p)] for g in opt.param_groups for p in g["params"]}
        assert grouped == self.grouped, sorted(grouped ^ self.grouped)[:4]
        self.model, self.opt = model, opt


def record(model: torch.nn.Module, opt, step: Callable[[], torch.Tensor], n: int,
           before: Callable[[int], None] = lambda t: None, into: Optional[Trajectory] = None) -> Trajectory:
    """``n`` times ``before(t); loss = step()``, a snapshot after each"""
    traj = Trajectory(model, opt) if into is None else into
    first = len(traj.steps)
    for t in range(first, first + n):
        before(t)
        traj.add(step())
    return traj


def _same(a: Optional[torch.Tensor], b: Optional[torch.Tensor]) -> bool:
    if a is None or b is None:
        return a is None and b is None
    if a.device != b.device:
        a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def compare(a: Trajectory, b: Trajectory, kinds=KINDS) -> List[Entry]:
    """the (step, kind, name) entries of the two trajectories that are not torch.equal (one missing or None counts), in
    the order of the steps"""
    assert len(a.steps) == len(b.steps) and a.steps, (len(a.steps), len(b.steps))
    out = []
    for t, (ra, rb) in enumerate(zip(a.steps, b.steps)):
        for kind in kinds:
            names = list(ra[kind]) + [n for n in rb[kind] if n not in ra[kind]]
            absent = object()
            for n in names:
                va, vb = ra[kind].get(n, absent), rb[kind].get(n, absent)
                if va is absent or vb is absent or not _same(va, vb):
                    out.append((t, kind, n))
    return out


def movement_violations(traj: Trajectory) -> List[Entry]:
    """(step, "unmoved", name): a grouped parameter with a non-zero gradient that the step left bitwise unchanged;
    (step, "moved-ungrouped", name): a parameter in no group that differs from its value before the first step"""
    out = []
    prev = traj.start
    for t, rec in enumerate(traj.steps):
        for n, p in rec["param"].items():
            if n in traj.grouped:
                g = rec["grad"][n]
                if g is not None and bool(g.any()) and _same(p, prev["param"][n]):
                    out.append((t, "unmoved", n))
            elif not _same(p, traj.start["param"][n]):
                out.append((t, "moved-ungrouped", n))
        prev = rec
    return out


def describe(entries: List[Entry], limit: int = 12) -> str:
    return "\n".join(f"  step {t}: {kind:<10s} {name}" for t, kind, name in entries[:limit]) + \
        (f"\n  ... {len(entries) - limit} more" if len(entries) > limit else "")
