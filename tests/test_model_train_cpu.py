"""The training-mode model against the reference's own model with GIVEN stochastic-depth masks, without a GPU:
the fixtures themselves (tests/golden/make_golden_model_train.py), the product's DropPath names and rates, and the
product's host logic on the CPU with the oracle scan and the fixture's masks injected into its one draw
(tests/model_utils.inject_masks).  The HIP path meets the same fixtures in tests/test_model_train_gpu.py."""
import numpy as np
import pytest
import torch

from tests.deepsup_utils import build_ds_model
from tests.model_utils import (assert_logits_close, build_model, digest, fill, inject_masks, load_mask_table, load_model_golden,
                               train_structure_violations)
from tests.oracle_backend import use_oracle_scan

import make_golden_model_train as gen        # tests/golden (on sys.path through tests.model_utils): reads no reference here

CASES = ["tiny_72x88_b2_train", "tiny_64x96_ds_train"]


def _build(case):
    meta, z = load_model_golden(case)
    deep = any(".norm_ds." in str(n) for n in z["grad_names"])
    build = build_ds_model if deep else (lambda nc, H, W: build_model(meta["backbone"], nc, H, W))
    return meta, z, deep, build(meta["num_classes"], meta["H"], meta["W"])


@pytest.fixture(scope="module", params=CASES)
def built(request):
    return _build(request.param)


@pytest.mark.parametrize("case", CASES)
def test_fixture_masks_are_a_legal_draw_with_the_four_conditions(case):
    meta, z = load_model_golden(case)
    masks, probs, calls = z["masks"], z["dp_probs"], z["dp_calls"]
    names = [str(n) for n in z["dp_names"]]
    assert meta["batch"] == 2 and masks.shape == (len(names), 2, 2) and set(np.unique(masks)) <= {0, 1}
    assert ((probs >= 0) & (probs < 1)).all() and set(calls) == {1, 2}
    for n, p, k, m in zip(names, probs, calls, masks):
        assert k == (2 if ".vssm." in n else 1), n
        if p == 0:
            assert m.all(), n                                      # the reference's DropPath is the identity at rate 0
    cond = gen.conditions(names, probs, calls, masks)
    gen.assert_conditions(cond)
    # the conditions as the issue words them, on the witnesses themselves
    by = dict(zip(names, masks))
    for stage, ws in cond["a"].items():
        rgb, x = by[ws[0]]
        assert f".vssm.layers.{stage}." in ws[0] and (rgb + x == 1).all() and rgb[0] != rgb[1]
    assert ".vssm.layers.3." in cond["b"][0] and by[cond["b"][0]].sum() == 0
    assert by[cond["c"][0]].all() and probs[names.index(cond["c"][0])] > 0
    assert sorted(cond["d"]) == [1, 2, 3] and all(by[ws[0]][0].sum() == 1 for ws in cond["d"].values())
    assert len(z["terms"]) == (4 if "_ds" in case else 1)
    assert abs(float(z["terms"].sum()) - float(z["loss"])) <= 4 * 2.0 ** -24 * float(z["loss"])


def test_drop_path_names_and_rates_are_the_references(built):
    """the module names of the product's DropPath layers and the rate of each against what the reference built: its
    torch.linspace over the encoder's 15 blocks and over the decoder's 16, sliced per level, and 0 in the fusion blocks"""
    from sigma_amd.models.encoders.vmamba import DropPath
    meta, z, deep, model = built
    table, probs = load_mask_table(z)
    got = {n: m.drop_prob for n, m in model.named_modules() if isinstance(m, DropPath)}
    assert sorted(got) == sorted(probs)
    for n, p in probs.items():
        # both sides take float32 linspace values through .item(): equal up to the rounding of one float32 step
        assert abs(got[n] - p) <= 2.0 ** -24 * max(p, 2.0 ** -10), (n, got[n], p)
    # 15 encoder blocks and 3 x 4 decoder blocks, the first of each linspace at rate 0; 12 fusion modules at rate 0
    assert sum(p > 0 for p in probs.values()) == 14 + 11 and len(probs) == 15 + 12 + 12
    assert max(probs.values()) == pytest.approx(0.2, abs=1e-7)


def test_host_model_logic_in_training_mode_matches_reference(built):
    """test_host_model_logic_matches_reference (tests/test_oracle_model.py) in ``train()`` with the fixture's masks: logits,
    loss, loss terms and EVERY parameter gradient, with that test's tolerances; then what dropped samples look like exactly"""
    meta, z, deep, model = built
    model.train()
    table, probs = load_mask_table(z)
    rgb, x, label = fill.make_inputs(meta["batch"], meta["H"], meta["W"], meta["num_classes"])
    assert torch.equal(label, torch.from_numpy(z["label"].astype(np.int64)))
    with use_oracle_scan():
        with torch.no_grad(), inject_masks(model, table, probs) as asked:
            logits = model(rgb, x)
        assert all(k == (probs[n] > 0) for n, k in asked.items()), asked
        assert_logits_close(logits, torch.from_numpy(z["logits"]), 2e-5)
        if deep:
            with torch.no_grad(), inject_masks(model, table, probs):
                outs = model.encode_decode(rgb, x)
            for o, r in zip(outs, z["terms"]):
                assert abs(float(model.criterion(o, label)) - float(r)) < 1e-4

        def step():
            with inject_masks(model, table, probs):
                loss = model(rgb, x, label)
            assert abs(loss.item() - float(z["loss"])) < 1e-4
            loss.backward()

        assert train_structure_violations(model, z, step) == []
    got = dict(model.named_parameters())
    assert sorted(str(n) for n in z["grad_names"]) == sorted(got)
    bad = []
    for n, r in zip(list(z["grad_names"]), z["grad_digest"]):
        g = got[str(n)].grad
        assert g is not None, n
        d = digest(g)
        if not np.allclose(d, r, rtol=2e-3, atol=2e-3 * (abs(r[1]) / max(g.numel(), 1) + 1e-6) * g.numel() ** 0.5 + 1e-6):
            bad.append((str(n), d, r))
    assert not bad, bad[:5]
    worst = []
    for i, n in enumerate(list(z["grad_full_names"])):
        r = torch.from_numpy(z[f"grad_full_{i}"])
        err = float((got[str(n)].grad - r).abs().max()) / (float(r.abs().max()) + 2e-5)
        if err > 5e-3:                                             # the element-wise bound of the GPU comparison, fp32 GEMMs
            worst.append((str(n), err))
    assert not worst, worst[:5]


def test_injection_refuses_a_second_draw_and_an_idle_module():
    from sigma_amd.models.encoders.vmamba import DropPath

    class Two(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = DropPath(0.25), DropPath(0.5)

    net = Two().train()
    table = {"a": [torch.tensor([1.0, 0.0])], "b": [torch.tensor([0.0]), torch.tensor([1.0])]}
    probs = {"a": 0.25, "b": 0.5}
    x = torch.ones(2, 3)
    with inject_masks(net, table, probs):
        assert torch.equal(net.a(x), torch.tensor([[1 / 0.75] * 3, [0.0] * 3]))        # the module's own 1 / keep
        assert torch.equal(net.b.draw(x).flatten(), torch.tensor([0.0, 2.0]))          # cat(call 0, call 1)
    with pytest.raises(AssertionError, match="more often"):
        with inject_masks(net, table, probs, may_skip=("b",)):
            net.a(x), net.a.add_to(x, x)
    with pytest.raises(AssertionError, match="never asked"):
        with inject_masks(net, table, probs):
            net.a(x)
    with pytest.raises(AssertionError, match="3 samples"):
        with inject_masks(net, table, probs, may_skip=("a",)):
            net.b(torch.ones(3, 1))
    assert DropPath.draw_mask.__name__ == "draw_mask"                                # restored
