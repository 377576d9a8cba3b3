"""The training-mode model on the HIP path -- run with -m gpu.

The step every user and the benchmark run is ``model.train()``: each encoder VSSBlock and each decoder CVSSDecoderBlock
draws a per-sample stochastic-depth mask that the product folds into its fused kernels (the row factor of the gated
LayerNorm, the residual of the out_proj GEMM, addcmul in the fusion blocks).  Checker: the REFERENCE's own model in
``train()`` under a given mask table (tests/golden/make_golden_model_train.py); the product gets the same masks through its
one draw (tests/model_utils.inject_masks) and applies its own rates, 1 / keep and folds.  Then what no tolerance can hide:
dropped samples bit for bit, wrong variants that must be noticed, fresh masks in a captured step, the draw's
statistics."""
import copy

import pytest
import torch

from tests.model_utils import (build_model, compare_with_reference_fixtures, fill, inject_masks, load_mask_table,
                               load_model_golden, product_block, shift_stage3, swap_modalities, train_structure_violations)

pytestmark = pytest.mark.gpu

CASES = ["tiny_72x88_b2_train", "tiny_64x96_ds_train"]
A_BLOCK = "backbone.vssm.layers.3.blocks.0.drop_path"      # a condition-(a) block, rate 0.2 * 13 / 14: 1 / keep = 1.23


@pytest.fixture
def gemm_mode(request, monkeypatch):
    """'fp32' = vendor fp32 GEMMs for every nn.Linear (the reference's arithmetic), 'split3' = the split-operand MFMA
    kernels (the default of the benchmark)"""
    monkeypatch.setenv("SIGMA_GEMM", request.param)
    return request.param


@pytest.mark.parametrize("gemm_mode", ["fp32", "split3"], indirect=True)
@pytest.mark.parametrize("case", CASES)
def test_training_mode_logits_loss_and_grads_match_reference_fixtures(case, gemm_mode):
    """tests/test_model_gpu.py::test_logits_loss_and_grads_match_reference_fixtures in ``train()`` with the fixture's masks,
    with its tolerances unchanged: logits 1e-3 of the logit scale, loss (and each deep-supervision term) 1e-3, gradient
    digests 5e-3 of the L1 mass, element-wise gradients 5e-3 (fp32 GEMMs) / 1e-2 (split-operand GEMMs) of the tensor's
    scale"""
    _, z = load_model_golden(case)
    compare_with_reference_fixtures(case, gemm_mode, masks=load_mask_table(z)[0])


@pytest.mark.parametrize("gemm_mode", ["fp32", "split3"], indirect=True)
@pytest.mark.parametrize("case", CASES)
def test_dropped_samples_pass_through_bit_for_bit(case, gemm_mode):
    """tests/model_utils.train_structure_violations on the HIP path: an encoder block returns a dropped sample's input bit
    for bit (the factor 0 reaches the out_proj GEMM as zero rows, whose accumulators start from the residual), the block
    that drops all four (image, modality) samples has gradients that are exactly 0.0, and a decoder block's SS2D branch is
    exactly 0 for a dropped sample"""
    from tests.deepsup_utils import build_ds_model
    meta, z = load_model_golden(case)
    build = build_ds_model if "_ds_" in case else (lambda nc, H, W: build_model(meta["backbone"], nc, H, W))
    model = build(meta["num_classes"], meta["H"], meta["W"]).cuda().train()
    table, probs = load_mask_table(z)
    rgb, x, label = (t.cuda() for t in fill.make_inputs(meta["batch"], meta["H"], meta["W"], meta["num_classes"]))

    def step():
        with inject_masks(model, table, probs):
            loss = model(rgb, x, label)
        loss.backward()

    assert train_structure_violations(model, z, step) == []


def _without_keep_scale(model):
    # the rate of one condition-(a) block so small that keep = 1 - rate rounds to 1 in float32: the block still draws and
    # applies its 0 / 1 mask, and 1 / keep is gone
    product_block(model, A_BLOCK).drop_path.drop_prob = 1e-12


def _rate_zero(model):
    product_block(model, A_BLOCK).drop_path.drop_prob = 0.0


VARIANTS = {
    "rgb-x-swapped": dict(table=swap_modalities),
    "shifted-in-stage-3": dict(table=shift_stage3),
    "no-keep-scale": dict(prepare=_without_keep_scale),
    "rate-0-block": dict(prepare=_rate_zero, may_skip=(A_BLOCK,)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_wrong_variants_are_noticed(variant, monkeypatch):
    """negative controls of the comparison above (same function, collecting its violations): the table with the RGB and X
    halves exchanged, the table shifted by one block within stage 3, 0 / 1 factors without 1 / keep on one block (its rate
    made negligible, so that the module still draws; and its rate set to 0, which also stops the draw)"""
    monkeypatch.setenv("SIGMA_GEMM", "fp32")
    case = CASES[0]
    _, z = load_model_golden(case)
    table = load_mask_table(z)[0]
    v = VARIANTS[variant]
    found = []
    compare_with_reference_fixtures(case, "fp32", masks=v.get("table", lambda t: t)(table), prepare=v.get("prepare"),
                                    may_skip=v.get("may_skip", ()), violations=found)
    print(variant, len(found), [str(f)[:160] for f in found[:3]])
    assert len(found) >= 1


def test_captured_training_step_draws_fresh_masks_at_every_replay():
    """sigma_amd.train_step.make_graphed_step on a ``train()`` model whose parameters cannot move (learning rate 0 through
    set_lr, weight decay 0): six replays on the same static batch do not all give the same loss -- the masks are drawn
    at replay time, not frozen into the graph -- and with the generator seeded just before it a replay gives the loss of
    the eager training-mode step from the same seed (tolerance of test_hip_graph_replay_equals_eager_step)."""
    from sigma_amd import train_step as ts
    dev = torch.device("cuda", 0)
    eager = build_model("sigma_tiny", 9, 64, 96).to(dev).train()
    graphed = copy.deepcopy(eager)
    batch = tuple(t.to(dev) for t in fill.make_inputs(2, 64, 96, 9, seed=8))
    opt_e = ts.make_optimizer(eager, weight_decay=0.0, capturable=True)
    opt_g = ts.make_optimizer(graphed, weight_decay=0.0, capturable=True)
    ts.set_lr(opt_e, 0.0)
    ts.set_lr(opt_g, 0.0)
    step_e = ts.make_step(eager, opt_e, batch)
    step_g, _ = ts.make_graphed_step(graphed, opt_g, batch, warmup=3)
    losses = []
    for _ in range(6):
        losses.append(step_g().detach().clone())
    torch.cuda.synchronize()
    losses = [float(l) for l in losses]
    print("replayed losses", losses)
    assert all(l == l for l in losses) and len(set(losses)) > 1, losses
    for (n, a), (_, b) in zip(eager.named_parameters(), graphed.named_parameters()):
        assert torch.equal(a, b), n                     # rate 0, decay 0: the replays left the parameters where they were
    for seed in (11, 12):
        torch.cuda.manual_seed(seed)
        lg = step_g().detach().clone()
        torch.cuda.manual_seed(seed)
        le = step_e().detach()
        torch.cuda.synchronize()
        print("seed", seed, "replay", float(lg), "eager", float(le))
        torch.testing.assert_close(lg, le, rtol=1e-5, atol=1e-6)


def test_the_draw_is_a_per_sample_bernoulli_scaled_by_keep():
    """8192 samples at rate 0.3 through DropPath.draw, add_to and forward: values in {0, 1 / keep}, one value per sample
    broadcast over the other dimensions, kept count within 5 standard deviations of the binomial mean"""
    from sigma_amd.models.encoders.vmamba import DropPath
    n, rate = 8192, 0.3
    keep = 1.0 - rate
    dp = DropPath(rate).train()
    torch.cuda.manual_seed(5)
    x = torch.ones(n, 3, 5, device="cuda")
    one = torch.ones((), device="cuda").div_(keep)      # 1 / keep as the module's own div_ rounds it
    assert abs(float(one) - 1.0 / keep) < 1e-6
    mean, sd = n * keep, (n * keep * rate) ** 0.5
    for how, out in (("draw", dp.draw(x).expand_as(x)), ("add_to", dp.add_to(torch.zeros_like(x), x)), ("forward", dp(x))):
        assert out.shape == x.shape, how
        assert bool(((out == 0) | (out == one)).all()), how
        assert bool((out == out[:, :1, :1]).all()), how
        kept = int((out[:, 0, 0] != 0).sum())
        print(how, "kept", kept, "mean", mean, "5 sd", 5 * sd)
        assert abs(kept - mean) <= 5 * sd, (how, kept)
    assert tuple(dp.draw(x).shape) == (n, 1, 1)
    assert dp.eval().draw(x) is None and DropPath(0.0).train().draw(x) is None
