#!/usr/bin/env python3
"""Generate the TRAINING-MODE model fixtures by running the REFERENCE's own Python model on CPU with given masks.

Run in the build container only (needs the reference checkout, read-only):

    python tests/golden/make_golden_model_train.py

As make_golden_model.py / make_golden_deepsup.py (same stubs, imported from them; nothing of the reference is copied), in
``model.train()``.  ``timm.models.layers.DropPath`` is the stub of make_golden_blocks.py, which multiplies by GIVEN
per-sample factors and counts its calls: the reference runs its encoder twice per step (dual_vmamba.py:85-86, RGB pass then
X pass), so every encoder DropPath is called twice, every fusion and decoder DropPath once.

Masks: a table keyed by (DropPath module name, call index) of 0/1 vectors of length B, drawn from a generator seeded by
the crc32 of the key with P(drop) = 0.5 where the module's drop_prob is above 0, all ones where it is 0 (timm returns its
input there).  Any pattern is a legal outcome of timm's draw.  Entries are then overridden so that the table holds
conditions (a) - (d) of ``conditions``.  The stub applies mask / (1 - drop_prob) with the REFERENCE module's drop_prob.

Outputs: tests/golden/model_<case>_train.npz
    dp_names / dp_probs / dp_calls   every DropPath module, its drop_prob in the reference, its calls per step
    masks                            (modules, 2, B) uint8, [m, c] = the mask of call c (rows past dp_calls[m] hold 1)
    logits                           training-mode logits (x_last) of a label-free forward under the table
    label, loss, terms               the label, the loss and (deep supervision) its four terms
    grad_names / grad_digest         digests of every parameter's gradient
    grad_full_names / grad_full_{k}  full gradients: the set of the eval fixture of the same model
"""
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fill  # noqa: E402
from make_golden_blocks import GivenDropPath  # noqa: E402
from make_golden_model import digest, full_gradient_names, install_stubs  # noqa: E402

CASES = [
    dict(name="tiny_72x88_b2_train", backbone="sigma_tiny", num_classes=5, H=72, W=88, batch=2, deep=False),   # odd stage sizes
    dict(name="tiny_64x96_ds_train", backbone="sigma_tiny", num_classes=9, H=64, W=96, batch=2, deep=True),
]

ENC = "backbone.vssm.layers.{}.blocks.{}.drop_path"
DEC = "decode_head.layers_up.{}.blocks.{}.drop_path"


def drawn_mask(name, call, batch, drop_prob):
    if drop_prob == 0:
        return np.ones(batch, np.uint8)
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}#{call}".encode()) & 0x7FFFFFFF)
    return (torch.rand(batch, generator=g) >= 0.5).numpy().astype(np.uint8)


def overrides(names):
    """(module name, call) -> mask for batch 2, written over the drawn table; `names` = the model's DropPath modules"""
    o = {}
    for stage, blk in ((0, 1), (1, 0), (2, 0), (3, 0)):           # (a); block 0 of stage 0 has rate 0
        o[ENC.format(stage, blk), 0] = [0, 1]                      # RGB pass: image 0 dropped
        o[ENC.format(stage, blk), 1] = [1, 0]                      # X pass: image 1 dropped
    o[ENC.format(3, 1), 0] = o[ENC.format(3, 1), 1] = [0, 0]       # (b)
    o[ENC.format(2, 4), 0] = o[ENC.format(2, 4), 1] = [1, 1]       # (c)
    for level, m in ((1, [0, 1]), (2, [1, 0]), (3, [0, 1])):      # (d)
        o[DEC.format(level, 1), 0] = m
    assert all(n in names for n, _ in o), sorted(set(n for n, _ in o) - set(names))
    return o


def conditions(names, probs, calls, masks):
    """The four conditions on a (modules, 2, B = 2) table, each as the list of module names that witness it:
      a  per encoder stage: a block where one image has its RGB call dropped and its X call kept, the other the reverse
      b  stage-3 blocks with all four (image, modality) entries dropped
      c  blocks with a non-zero rate and nothing dropped
      d  per decoder level with a non-zero rate: a block that drops exactly one of the two images"""
    def index_after(n, word):
        parts = n.split(".")
        return int(parts[parts.index(word) + 1])

    a, b, c = {}, [], []
    d = {index_after(str(n), "layers_up"): [] for n, p in zip(names, probs) if ".layers_up." in str(n) and p > 0}
    for n, p, k, m in zip(names, probs, calls, masks):
        n, m = str(n), m[:k].astype(int)
        if p > 0 and m.all():
            c.append(n)
        if ".vssm.layers." in n:
            stage = index_after(n, "layers")
            a.setdefault(stage, [])
            if k == 2 and sorted(map(tuple, m.T.tolist())) == [(0, 1), (1, 0)]:      # a column is one image: (RGB, X)
                a[stage].append(n)
            if stage == 3 and k == 2 and not m.any():
                b.append(n)
        if ".layers_up." in n and p > 0 and m[0].sum() == 1:
            d[index_after(n, "layers_up")].append(n)
    return dict(a=a, b=b, c=c, d=d)


def assert_conditions(cond):
    assert sorted(cond["a"]) == [0, 1, 2, 3] and all(cond["a"][s] for s in cond["a"]), cond["a"]
    assert cond["b"], "no stage-3 block with everything dropped"
    assert cond["c"], "no block with a non-zero rate and nothing dropped"
    assert cond["d"] and all(cond["d"][lv] for lv in cond["d"]), cond["d"]


def build(c):
    from models.builder import EncoderDecoder
    cfg = types.SimpleNamespace(backbone=c["backbone"], decoder="MambaDecoder", num_classes=c["num_classes"],
                                image_height=c["H"], image_width=c["W"], pretrained_model=None, bn_eps=1e-3,
                                bn_momentum=0.1, decoder_embed_dim=512)
    torch.manual_seed(0)
    crit = torch.nn.CrossEntropyLoss(reduction="mean", ignore_index=255)
    model = EncoderDecoder(cfg=cfg, criterion=crit, norm_layer=torch.nn.BatchNorm2d)
    if c["deep"]:                                                  # as make_golden_deepsup.py
        from models.decoders.MambaDecoder import MambaDecoder
        model.decode_head = MambaDecoder(img_size=[c["H"], c["W"]], in_channels=model.channels, num_classes=c["num_classes"],
                                         embed_dim=model.channels[0], deep_supervision=True)
        model.deep_supervision = True
        model.init_weights(cfg, pretrained=None)
    fill.fill_parameters(model)
    return model.train(), crit


def run_case(c):
    model, crit = build(c)
    B = c["batch"]
    rgb, x, label = fill.make_inputs(B, c["H"], c["W"], c["num_classes"])
    dps = [(n, m) for n, m in model.named_modules() if isinstance(m, GivenDropPath)]
    names = [n for n, _ in dps]

    def reset():
        for _, m in dps:
            m.calls = 0

    with torch.no_grad():                                          # count the calls of a step: no factors yet
        model(rgb, x)
    calls = [m.calls for _, m in dps]
    assert set(calls) <= {1, 2} and all((k == 2) == (".vssm." in n) for n, k in zip(names, calls))
    probs = [float(m.drop_prob) for _, m in dps]
    masks = np.ones((len(dps), 2, B), np.uint8)
    over = overrides(names)
    for i, (n, m) in enumerate(dps):
        for call in range(calls[i]):
            masks[i, call] = over.get((n, call), drawn_mask(n, call, B, probs[i]))
        if probs[i] == 0:
            assert masks[i].all(), n                               # timm: identity at rate 0
        m.factors = [torch.from_numpy(masks[i, call].astype(np.float32)) / (1.0 - probs[i]) for call in range(calls[i])]
    assert set(np.unique(masks)) <= {0, 1}
    cond = conditions(names, probs, calls, masks)
    assert_conditions(cond)

    reset()
    with torch.no_grad():
        logits = model(rgb, x)
    assert [m.calls for _, m in dps] == calls
    reset()
    if c["deep"]:
        outs = model.encode_decode(rgb, x)
        terms = [crit(o, label.long()) for o in outs]
        loss = terms[0] + terms[1] + terms[2] + terms[3]
        assert torch.equal(outs[0].detach(), logits)
    else:
        loss = model(rgb, x, label)
        terms = [loss]
    loss.backward()
    assert [m.calls for _, m in dps] == calls

    meta = {k: v for k, v in c.items() if k != "deep"}
    blob = {"meta": np.array(repr(meta)), "dp_names": np.array(names), "dp_probs": np.array(probs, np.float64),
            "dp_calls": np.array(calls, np.int64), "masks": masks, "logits": logits.numpy(),
            "label": label.numpy().astype(np.int16), "loss": np.array(loss.item()),
            "terms": np.array([t.item() for t in terms])}
    gnames, gdig = [], []
    for n, p in model.named_parameters():
        gnames.append(n)
        gdig.append(digest(p.grad) if p.grad is not None else np.full(3, np.nan))
    blob["grad_names"] = np.array(gnames)
    blob["grad_digest"] = np.stack(gdig)
    if c["deep"]:
        full = [n for n, p in model.named_parameters() if ".norm_ds." in n or ".output_ds." in n]
    else:
        full = full_gradient_names(model)
    blob["grad_full_names"] = np.array(full)
    named = dict(model.named_parameters())
    for i, n in enumerate(full):
        blob[f"grad_full_{i}"] = named[n].grad.detach().numpy()
    path = os.path.join(HERE, f"model_{c['name']}.npz")
    np.savez_compressed(path, **blob)
    print(path, "loss %.6f" % loss.item(), "terms", [round(t.item(), 6) for t in terms], "dropped %d of %d entries" %
          (int(sum((1 - masks[i, :k]).sum() for i, k in enumerate(calls))), B * sum(calls)),
          "%.0f KiB" % (os.path.getsize(path) / 1024))
    print("  conditions:", {k: (v if isinstance(v, list) else {s: w[:1] for s, w in v.items()}) for k, v in cond.items()})


def main():
    install_stubs()
    sys.modules["timm.models.layers"].DropPath = GivenDropPath
    os.chdir("/tmp")
    for c in CASES:
        run_case(c)


if __name__ == "__main__":
    main()
