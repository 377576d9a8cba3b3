"""Child process of tests/test_distill_loss_gpu.py (``python -m tests.distill_capture_worker``): forward and backward of
``pointwise.DistillLossFn`` at 257 rows x 37 classes (student pitch 40, teacher pitch 44) captured with torch.cuda.graph,
replayed on new inputs, against the eager bytes of the same inputs; then a replay after the teacher's logits alone changed
in place.  In a process of its own, as tests/graph_step_worker.py: a capture mistake is an abort.  Exit 0 only when loss,
terms and the gradient of every replay equal the eager ones bit for bit."""
import sys

import torch

TAG = "[distill_capture_worker]"
ROWS, NC, LD, LDT, IGNORE = 257, 37, 40, 44, 255
ARGS = (IGNORE, LD, LDT, 2.0, 0.7, 0.5, True)            # ignore_index, ld, ld_t, T, kw, cw, kd_all


def say(msg):
    print(f"{TAG} {msg}", flush=True)


def step(xbuf, tbuf, lab, up):
    """(loss, terms, gradient) of one forward + backward with the upstream gradient `up` (a device scalar)"""
    from sigma_amd.pointwise import DistillLossFn
    leaf = xbuf.detach()[:, :NC].requires_grad_(True)
    loss, terms = DistillLossFn.apply(leaf, tbuf[:, :NC], lab, *ARGS)
    (g,) = torch.autograd.grad(loss, leaf, grad_outputs=up)
    return loss.detach(), terms, g


def main() -> int:
    from tests.distill_loss_bounds import distill_inputs
    dev = torch.device("cuda", 0)
    batches = [tuple(t.to(dev) for t in distill_inputs(ROWS, NC, LD, LDT, seed=s)) for s in (11, 12, 13)]
    ups = [torch.tensor(v, device=dev) for v in (1.0, -2.5, 0.37)]
    x, te, lab, up = batches[0][0].clone(), batches[0][1].clone(), batches[0][2].clone(), ups[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up off the default stream, as torch.cuda.graph asks
        step(x, te, lab, up)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step(x, te, lab, up)
    bad = 0
    for i, ((bx, bt, bl), bu) in enumerate(zip(batches, ups)):
        x.copy_(bx), te.copy_(bt), lab.copy_(bl), up.copy_(bu)
        graph.replay()
        got = [t.clone() for t in static]
        want = step(bx, bt, bl, bu)
        torch.cuda.synchronize()
        same = [torch.equal(a, b) for a, b in zip(got, want)]
        say(f"replay {i}: loss {float(got[0]):.6f}, (loss, terms, gradient) == eager: {same}")
        bad += not all(same)
        assert bool(torch.isfinite(got[2]).all()) and float(got[2].abs().max()) > 0
    # the teacher's logits alone change in place: the replay follows them
    before = [t.clone() for t in static]
    te[:, :NC].mul_(0.5).add_(0.25)
    graph.replay()
    got = [t.clone() for t in static]
    want = step(x, te, lab, up)
    torch.cuda.synchronize()
    same = [torch.equal(a, b) for a, b in zip(got, want)]
    moved = not torch.equal(got[0], before[0]) and not torch.equal(got[2], before[2]) and torch.equal(got[1][1], before[1][1])
    say(f"teacher changed in place: == eager: {same}, loss and gradient moved, cross entropy did not: {moved}")
    bad += not (all(same) and moved)
    say("done" if not bad else "FAILED")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
