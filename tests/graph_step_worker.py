"""Child process of tests/test_graph_step_gpu.py (``python -m tests.graph_step_worker SCENARIO``): the captured training
step of sigma_amd.train_step against the eager step, bit for bit, under torch.use_deterministic_algorithms(True) -- every
float atomic of the step is then replaced and the capture runs the kernels the eager step runs, so the
assertion is equality.  Model sigma_tiny, 9 classes, 64x96, batch 2; both sides
``make_optimizer(capturable=True)``; the eager replica takes the capture's warm-up steps (same batch, same rate); then
four compared steps, each on a new batch and at a new rate (``set_lr``), recorded with tests/train_trajectory.py: loss,
buffers, gradients, optimizer state and parameters after every step.

Scenarios: graph-eval, graph-train, graph-raw-params, graph-resume, ddp-fp32, ddp-bf16 and the negative control
float-lr-control (the docstrings below).  Exit 0 only when every comparison of the scenario holds; otherwise the first
differing (step, kind, name) entries are printed."""
import copy
import os
import socket
import sys
import tempfile
import time

import torch

from tests import train_trajectory as tt

TAG = "[graph_step_worker]"
SHAPE = dict(classes=9, H=64, W=96, batch=2)
WARMUP, WARM_BATCH, WARM_RATE, WARM_SEED = 2, 100, 6e-5, 99
STEPS = 4
RATES = [1.5e-5, 3e-5, 6e-5, 4.2e-5]                 # neighbours differ by at least 1.4x: a stale rate is unmistakable
SEEDS = [1001, 1002, 1003, 1004]                     # torch.cuda.manual_seed just before step t (train mode: DropPath)


def say(msg):
    print(f"{TAG} {msg}", flush=True)


def replica(base, raw=False):
    """(a deep copy of ``base``, its optimizer)"""
    from sigma_amd import train_step as ts
    model = copy.deepcopy(base)
    return model, ts.make_optimizer(model, lr=WARM_RATE, capturable=True, include_raw_params=raw)


def make_batch(dev, seed):
    from tests.model_utils import fill
    return tuple(t.to(dev) for t in fill.make_inputs(SHAPE["batch"], SHAPE["H"], SHAPE["W"], SHAPE["classes"], seed=seed))


class Side:
    """one replica: model, optimizer, the step to call and how a batch and a rate reach it"""

    def __init__(self, model, opt):
        from sigma_amd import train_step as ts
        self.ts, self.model, self.opt = ts, model, opt
        self.dev = next(model.parameters()).device

    def batch(self, seed):
        return make_batch(self.dev, seed)


class Eager(Side):
    """train_step.make_step's sequence; ``wire``: the data-parallel loop of tests/graph_ddp_worker.py (loss all-reduce,
    per-parameter gradient all-reduce; "bf16": each gradient through bf16 and back, the flat buffer's round trip).

    ``optimizer.zero_grad()`` clears what the optimizer owns: the gradients of the parameters in no group add up from
    step to step, here as in the reference and in make_graphed_step, and nothing reads them.  make_graphed_ddp_step zeroes
    its whole flat buffer instead, so the data-parallel loop clears every gradient (``drop_gradients``) before a step: each
    side then holds the gradient of one step, which can be compared."""

    def __init__(self, base, raw=False, wire=None):
        super().__init__(*replica(base, raw))
        self.wire, self.cur = wire, None
        self.warm_up(WARMUP, self.batch(WARM_BATCH))

    def warm_up(self, n, batch):
        torch.cuda.manual_seed(WARM_SEED)
        self.cur = batch
        for _ in range(n):
            self.step()

    def drop_gradients(self):
        for p in self.model.parameters():
            p.grad = None

    def step(self):
        import torch.distributed as dist
        if self.wire is not None:
            self.drop_gradients()
        self.opt.zero_grad(set_to_none=True)
        loss = self.model(*self.cur)
        if self.wire is not None:
            red = loss.detach().clone()
            dist.all_reduce(red)
        loss.backward()
        if self.wire is not None:
            for p in self.model.parameters():
                dist.all_reduce(p.grad)                  # world size 1: one addend, no division
                if self.wire == "bf16":
                    p.grad.copy_(p.grad.to(torch.bfloat16).float())
        self.opt.step()
        return loss

    def before(self, t):
        self.cur = self.batch(t)
        self.ts.set_lr(self.opt, RATES[t])
        torch.cuda.manual_seed(SEEDS[t])


class Graphed(Side):
    """make_graphed_step, or with ``wire`` make_graphed_ddp_step, captured on the warm-up batch at the warm-up rate"""

    def __init__(self, model, opt, wire=None, float_lr=False, warmup=WARMUP, warm_batch=WARM_BATCH):
        super().__init__(model, opt)
        self.float_lr = float_lr
        torch.cuda.manual_seed(WARM_SEED)
        warm = self.batch(warm_batch)
        if wire is None:
            self.step, self.static = self.ts.make_graphed_step(self.model, self.opt, warm, warmup=warmup)
        else:
            self.step, self.static = self.ts.make_graphed_ddp_step(self.model, self.opt, warm, warmup=warmup, bf16_comm=wire == "bf16")

    def before(self, t):
        for s, v in zip(self.static, self.batch(t)):
            s.copy_(v)
        if self.float_lr:                                # the negative control: a replay cannot see this
            for g in self.opt.param_groups:
                g["lr"] = RATES[t]
        else:
            self.step.set_lr(RATES[t])
        torch.cuda.manual_seed(SEEDS[t])


def verdict(what, entries, good="equal") -> int:
    if entries:
        say(f"{what}: {len(entries)} entries, the first:\n{tt.describe(entries)}")
        return 1
    say(f"{what}: {good}")
    return 0


def moved(traj) -> int:
    n_free = len(traj.start["param"]) - len(traj.grouped)
    say(f"{len(traj.grouped)} parameters in optimizer groups, {n_free} in none")
    return verdict("movement on the eager side (grouped parameters move at every step, the others never)",
                   tt.movement_violations(traj), good="holds")


def graph_plain(base, raw=False, wire=None) -> int:
    """graph-eval / graph-train / ddp-*: the whole trajectory of the captured step equals the eager one"""
    e = Eager(base, raw, wire)
    te = tt.record(e.model, e.opt, e.step, STEPS, e.before)
    g = Graphed(*replica(base, raw), wire=wire)
    bad = 0
    if wire is None:
        tg = tt.record(g.model, g.opt, g.step, STEPS, g.before)
    else:
        same = []

        def step():
            loss = g.step()
            same.append(torch.equal(g.step.reduced_loss, loss.detach()))
            return loss
        tg = tt.record(g.model, g.opt, step, STEPS, g.before)
        say(f"step.reduced_loss == loss at every step: {same}")
        bad += not all(same)
    torch.cuda.synchronize()
    assert ts_unoptimized(e) == ts_unoptimized(g) == len(te.start["param"]) - len(te.grouped)
    bad += verdict("captured against eager", tt.compare(te, tg))
    bad += moved(te)
    say(f"losses {[round(float(r['loss']['loss']), 6) for r in tg.steps]}")
    del g
    return bad


def ts_unoptimized(side) -> int:
    return side.ts.unoptimized_parameters(side.model, side.opt.param_groups)


def graph_raw_params(base) -> int:
    """include_raw_params=True: the optimizer owns the raw Mamba parameters, so the SS2D blocks' cached derived tensors
    (ss2d_fused._derived_params) go stale with every step.  A validation forward (eager, no_grad) after two steps fills
    the cache; two more steps; then the same forward must see the stepped parameters: it equals, bitwise, the forward of a
    deep copy taken after invalidate_derived_params().  Both forwards and the whole trajectory equal the eager side's."""
    from sigma_amd.ss2d_fused import invalidate_derived_params
    trajs, logits = [], []
    for graphed in (False, True):
        s = Graphed(*replica(base, raw=True)) if graphed else Eager(base, raw=True)
        assert ts_unoptimized(s) == 0
        val = s.batch(500)[:2]
        t = tt.record(s.model, s.opt, s.step, 2, s.before)
        with torch.no_grad():
            mid = s.model(*val).clone()
        tt.record(s.model, s.opt, s.step, 2, s.before, into=t)
        with torch.no_grad():
            end = s.model(*val).clone()
        invalidate_derived_params()
        with torch.no_grad():
            fresh = copy.deepcopy(s.model)(*val)
        trajs.append(t), logits.append((mid, end, fresh))
    torch.cuda.synchronize()
    bad = 0
    for name, (mid, end, fresh) in zip(("eager", "captured"), logits):
        ok = torch.equal(end, fresh)
        say(f"{name}: forward after the steps == forward of a fresh copy: {ok}"
            + ("" if ok else f" (max |diff| {(end - fresh).abs().max().item():.3e})"))
        bad += not ok
        assert not torch.equal(mid, end)                 # the two steps in between did change what the forward computes
    ok = torch.equal(logits[0][0], logits[1][0]) and torch.equal(logits[0][1], logits[1][1])
    say(f"validation logits, captured == eager: {ok}")
    bad += not ok
    bad += verdict("captured against eager", tt.compare(trajs[0], trajs[1]))
    bad += moved(trajs[0])
    return bad


def graph_resume(base) -> int:
    """warm-up + two replays; model and optimizer state_dict through torch.save / torch.load(map_location="cpu") into a
    fresh model and a fresh optimizer; a new captured step (one warm-up step on the next batch at the restored rate); two
    more steps.  Equal to an uninterrupted eager run of the same batches and rates (which drops its gradients where the
    other side restarts: a checkpoint holds none, and those of the parameters in no group would go on adding up).  After the resume every group's rate
    is a tensor on the parameters' device (train_step._tensor_lrs moves the CPU tensor load_state_dict leaves there)."""
    from tests.model_utils import build_model
    e = Eager(base)
    te = tt.record(e.model, e.opt, e.step, 2, e.before)
    e.drop_gradients()
    e.warm_up(1, e.batch(2))
    tt.record(e.model, e.opt, e.step, 2, e.before, into=te)

    g = Graphed(*replica(base))
    tg = tt.record(g.model, g.opt, g.step, 2, g.before)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ckpt.pt")
        torch.save(dict(model=g.model.state_dict(), opt=g.opt.state_dict()), path)
        ckpt = torch.load(path, map_location="cpu")
    dev, ts = g.dev, g.ts
    del g
    model = build_model("sigma_tiny", SHAPE["classes"], SHAPE["H"], SHAPE["W"]).to(dev).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)                                  # nothing of the fresh model may survive the load
    opt = ts.make_optimizer(model, lr=WARM_RATE, capturable=True)
    model.load_state_dict(ckpt["model"])
    opt.load_state_dict(ckpt["opt"])
    say(f"after load_state_dict the rates are on {[str(g['lr'].device) if torch.is_tensor(g['lr']) else type(g['lr']).__name__ for g in opt.param_groups]}")
    r = Graphed(model, opt, warmup=1, warm_batch=2)
    bad = 0
    for i, grp in enumerate(opt.param_groups):
        ok = torch.is_tensor(grp["lr"]) and all(grp["lr"].device == p.device for p in grp["params"])
        ok = ok and float(grp["lr"]) == float(torch.tensor(RATES[1]))
        say(f"group {i}: rate {grp['lr']!r} on its parameters' device with the checkpoint's value: {ok}")
        bad += not ok
    tg.rebind(model, opt)
    tt.record(model, opt, r.step, 2, r.before, into=tg)
    torch.cuda.synchronize()
    bad += verdict("resumed captured run against the uninterrupted eager run", tt.compare(te, tg))
    bad += moved(te)
    return bad


def float_lr_control(base) -> int:
    """negative control on the real path: the captured side gets its rate as a Python float in param_groups[i]['lr'],
    which a replay cannot see (it goes on with the warm-up's rate); the eager side honours it.  The comparison must report
    the parameters -- and nothing else -- at step 0, whose rate is the first to differ, and the loss from step 1 on."""
    e = Eager(base)
    te = tt.record(e.model, e.opt, e.step, STEPS, e.before)
    g = Graphed(*replica(base), float_lr=True)
    tg = tt.record(g.model, g.opt, g.step, STEPS, g.before)
    torch.cuda.synchronize()
    diff = tt.compare(te, tg)
    at0 = {kind for t, kind, _ in diff if t == 0}
    names0 = {n for t, kind, n in diff if t == 0}
    later = [{kind for t, kind, _ in diff if t == s} for s in range(1, STEPS)]
    say(f"{len(diff)} differences; step 0: kinds {sorted(at0)}, {len(names0)} parameters of {len(te.grouped)} in groups; "
        f"later steps: {[sorted(k) for k in later]}")
    stepped = {n for n in te.grouped if not torch.equal(te.steps[0]["param"][n], te.start["param"][n])}
    ok = at0 == {"param"} and names0 == stepped and len(stepped) > 0 and all({"loss", "grad", "param", "exp_avg"} <= k for k in later)
    if not ok:
        say("the control was NOT reported as expected:\n" + tt.describe(diff))
        return 1
    say("control reported: differences from step 0")
    return moved(te)


def main(scenario: str) -> int:
    t0 = time.perf_counter()
    torch.use_deterministic_algorithms(True)
    torch.utils.deterministic.fill_uninitialized_memory = False
    from sigma_amd import deterministic_enabled
    from tests.model_utils import build_model
    assert deterministic_enabled() and os.environ.get("CUBLAS_WORKSPACE_CONFIG") == ":4096:8"
    dev = torch.device("cuda", 0)
    base = build_model("sigma_tiny", SHAPE["classes"], SHAPE["H"], SHAPE["W"]).to(dev)
    base.train(scenario == "graph-train")
    wire = {"ddp-fp32": "fp32", "ddp-bf16": "bf16"}.get(scenario)
    if wire is not None:
        import torch.distributed as dist
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("nccl", rank=0, world_size=1)
    if scenario in ("graph-eval", "graph-train", "ddp-fp32", "ddp-bf16"):
        bad = graph_plain(base, wire=wire)
    elif scenario == "graph-raw-params":
        bad = graph_raw_params(base)
    elif scenario == "graph-resume":
        bad = graph_resume(base)
    elif scenario == "float-lr-control":
        bad = float_lr_control(base)
    else:
        raise SystemExit(f"unknown scenario {scenario!r}")
    torch.cuda.synchronize()
    if wire is not None:
        import gc
        gc.collect()                                     # the captured graphs go before the communicator does
        dist.destroy_process_group()
    say(f"{scenario}: {time.perf_counter() - t0:.1f} s in the worker")
    if bad:
        return 1
    say(f"{scenario} done")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
