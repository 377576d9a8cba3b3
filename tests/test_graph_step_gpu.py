"""The captured training step of sigma_amd.train_step (make_graphed_step, make_graphed_ddp_step, set_lr, _tensor_lrs, the
optimizer groups) against the eager step, BIT FOR BIT, under torch's deterministic flag: losses, buffers,
gradients, AdamW state and parameters after each of four steps on new batches at new rates; an eager forward after
replays that stepped the raw Mamba parameters; a resume from a checkpoint read with map_location="cpu"; the two wire
formats of the data-parallel step on one rank; and a negative control on the real path (a float rate the replay cannot
see) that the same comparison must report.  One child process per scenario (tests/graph_step_worker.py): the flag and
CUBLAS_WORKSPACE_CONFIG stay out of this process, and a capture mistake next to a live communicator is an abort."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ["graph-eval", "graph-train", "graph-raw-params", "graph-resume", "ddp-fp32", "ddp-bf16", "float-lr-control"]
TIMEOUT = 60                                         # seconds per worker: 5x the slowest measured (11.5 s)
_ENDED_BADLY = []                                    # once a worker died or hung, nothing more is started on the device


def _run(scenario):
    if _ENDED_BADLY:
        pytest.fail(f"not started: the worker of {_ENDED_BADLY[0]}")
    env = dict(os.environ, CUBLAS_WORKSPACE_CONFIG=":4096:8")
    try:
        r = subprocess.run([sys.executable, "-m", "tests.graph_step_worker", scenario], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _ENDED_BADLY.append(f"{scenario} did not end within {TIMEOUT} s")
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"worker timed out after {TIMEOUT} s\n--- stdout\n{out[-3000:]}")
    if r.returncode < 0 or r.returncode in (134, 139):
        _ENDED_BADLY.append(f"{scenario} ended with status {r.returncode}")
    assert r.returncode == 0, f"worker exit {r.returncode}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    assert f"[graph_step_worker] {scenario} done" in r.stdout
    print(r.stdout[-2000:])
    return r.stdout


@pytest.mark.parametrize("scenario", SCENARIOS[:-1])
def test_captured_step_equals_eager_step_bitwise(scenario):
    out = _run(scenario)
    assert "captured against eager: equal" in out or "against the uninterrupted eager run: equal" in out
    assert "movement on the eager side (grouped parameters move at every step, the others never): holds" in out


def test_a_float_rate_the_replay_cannot_see_is_reported():
    """the negative control: the worker exits 0 only when the comparison reported the parameters at step 0 and nothing
    else there, and losses, gradients, moments and parameters at every later step"""
    assert "control reported: differences from step 0" in _run(SCENARIOS[-1])
