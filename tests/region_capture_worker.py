"""Child process of tests/test_region_loss_gpu.py (``python -m tests.region_capture_worker``): forward and backward of
``pointwise.RegionLossFn`` at 257 rows x 40 classes captured with torch.cuda.graph, replayed on new inputs, against the eager
bytes of the same inputs.  In a process of its own, as tests/graph_step_worker.py: a capture mistake is an abort.  Exit 0
only when loss, terms, sums and the gradient of every replay equal the eager ones bit for bit."""
import sys

import torch

TAG = "[region_capture_worker]"
ROWS, NC, IGNORE = 257, 40, 255
ARGS = (IGNORE, NC, 0.3, 0.7, 0.5, 0.8, 1.25)            # ignore_index, ld, a, b, s, rw, cw


def say(msg):
    print(f"{TAG} {msg}", flush=True)


def step(x, lab, up):
    """(loss, terms, sums, gradient) of one forward + backward with the upstream gradient `up` (a device scalar)"""
    from sigma_amd.pointwise import RegionLossFn
    leaf = x.detach().requires_grad_(True)
    loss, terms, sums = RegionLossFn.apply(leaf, lab, *ARGS)
    (g,) = torch.autograd.grad(loss, leaf, grad_outputs=up)
    return loss.detach(), terms, sums, g


def main() -> int:
    from tests.region_loss_bounds import region_inputs
    dev = torch.device("cuda", 0)
    batches = [tuple(t.to(dev) for t in region_inputs(ROWS, NC, NC, seed=s)) for s in (11, 12, 13)]
    ups = [torch.tensor(v, device=dev) for v in (1.0, -2.5, 0.37)]
    x, lab, up = batches[0][0].clone(), batches[0][1].clone(), ups[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up off the default stream, as torch.cuda.graph asks
        step(x, lab, up)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step(x, lab, up)
    bad = 0
    for i, ((bx, bl), bu) in enumerate(zip(batches, ups)):
        x.copy_(bx), lab.copy_(bl), up.copy_(bu)
        graph.replay()
        got = [t.clone() for t in static]
        want = step(bx, bl, bu)
        torch.cuda.synchronize()
        same = [torch.equal(a, b) for a, b in zip(got, want)]
        say(f"replay {i}: loss {float(got[0]):.6f}, (loss, terms, sums, gradient) == eager: {same}")
        bad += not all(same)
        assert bool(torch.isfinite(got[3]).all()) and float(got[3].abs().max()) > 0
    assert not torch.equal(static[3], step(*batches[0], ups[0])[3])          # the replays did see new inputs
    say("done" if not bad else "FAILED")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
