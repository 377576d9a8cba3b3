"""bench.py --dump-outputs: what the last timed step computed, bounded in size and sampled the same way every run."""
import os

import numpy as np
import torch
import torch.nn as nn

import bench


def _model(seed):
    torch.manual_seed(seed)
    m = nn.Sequential(nn.Linear(40, 30), nn.ReLU(), nn.Linear(30, 20))
    m[0].bias.requires_grad_(False)                    # frozen: not part of what the step updates
    m(torch.randn(8, 40)).square().mean().backward()
    return m


def _flat(m, grad):
    return torch.cat([(p.grad if grad else p).detach().reshape(-1) for p in m.parameters() if p.requires_grad]).numpy()


def test_small_model_is_dumped_whole(tmp_path):
    m = _model(0)
    out = bench.step_outputs(m, torch.tensor(1.25))
    assert sorted(out) == ["grads", "loss", "params"]
    np.testing.assert_array_equal(out["params"], _flat(m, False))
    np.testing.assert_array_equal(out["grads"], _flat(m, True))
    bench.dump_outputs(out, str(tmp_path / "d"))
    loaded = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert set(loaded) == set(out) and all(v.dtype == np.float32 for v in loaded.values())
    assert loaded["loss"].tolist() == [1.25]


def test_large_model_is_sampled_within_the_limit_at_fixed_indices():
    limit = 4 + 2 * 4 * 100                            # the loss and 100 elements of each vector
    a, b = _model(0), _model(1)
    oa, ob = bench.step_outputs(a, torch.tensor(0.5), limit), bench.step_outputs(b, torch.tensor(0.5), limit)
    assert sum(v.nbytes for v in oa.values()) <= limit
    assert oa["params"].size == oa["grads"].size == 100
    # the indices depend on the shapes alone: the sample of each model is the same selection of its flat vectors
    pa, pb = _flat(a, False), _flat(b, False)
    idx = [int(np.flatnonzero(pa == v)[0]) for v in oa["params"]]
    assert idx == sorted(set(idx))
    np.testing.assert_array_equal(ob["params"], pb[idx])
    np.testing.assert_array_equal(oa["grads"], _flat(a, True)[idx])
    np.testing.assert_array_equal(ob["grads"], _flat(b, True)[idx])
