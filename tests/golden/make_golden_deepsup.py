#!/usr/bin/env python3
"""Generate the deep-supervision fixture by running the REFERENCE's own Python model on CPU.

Run in the build container only (needs the reference checkout, read-only):

    python tests/golden/make_golden_deepsup.py

As make_golden_model.py (same stubs, imported from it; nothing of the reference is copied): the reference's
EncoderDecoder for sigma_tiny, 64x96, 9 classes, batch 1, with its ``decode_head`` replaced by the reference's own
``MambaDecoder(deep_supervision=True)`` and ``model.deep_supervision = True`` -- the one constant of models/builder.py:102
that keeps the branch of :141-144 / :158-166 from running.  Weights: fill.fill_parameters; inputs: fill.make_inputs.

Output: tests/golden/model_tiny_64x96_ds.npz
    keys                      sorted state-dict keys
    x_last                    (1, 9, 64, 96) in full
    aux{i}_digest / aux{i}_s4 digest of x_output_i and its rows / columns 0, 4, 8, ...
    coarse{i}                 norm_ds[i](y), the (1, h, w, C) map the head of level i reads, in full
    label, loss, terms        the label, the total loss and its four terms (x_last, x_output_0, 1, 2)
    grad_names / grad_digest  digests of every parameter's gradient
    grad_full_names / grad_full_{k}   full gradients of norm_ds.* and output_ds.*
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fill  # noqa: E402
from make_golden_model import digest, install_stubs  # noqa: E402

CASE = dict(name="tiny_64x96_ds", backbone="sigma_tiny", num_classes=9, H=64, W=96, batch=1)


def main():
    install_stubs()
    os.chdir("/tmp")
    from models.builder import EncoderDecoder
    from models.decoders.MambaDecoder import MambaDecoder
    c = CASE
    cfg = types.SimpleNamespace(backbone=c["backbone"], decoder="MambaDecoder", num_classes=c["num_classes"],
                                image_height=c["H"], image_width=c["W"], pretrained_model=None, bn_eps=1e-3,
                                bn_momentum=0.1, decoder_embed_dim=512)
    torch.manual_seed(0)
    crit = torch.nn.CrossEntropyLoss(reduction="mean", ignore_index=255)
    model = EncoderDecoder(cfg=cfg, criterion=crit, norm_layer=torch.nn.BatchNorm2d)
    model.decode_head = MambaDecoder(img_size=[c["H"], c["W"]], in_channels=model.channels, num_classes=c["num_classes"],
                                     embed_dim=model.channels[0], deep_supervision=True)
    model.deep_supervision = True
    model.init_weights(cfg, pretrained=None)
    fill.fill_parameters(model)
    model.eval()
    rgb, x, label = fill.make_inputs(c["batch"], c["H"], c["W"], c["num_classes"])
    coarse = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: coarse.append(out.detach().clone())) for m in model.decode_head.norm_ds]
    outs = model.encode_decode(rgb, x)
    for h in hooks:
        h.remove()
    terms = [crit(o, label.long()) for o in outs]
    loss = terms[0] + terms[1] + terms[2] + terms[3]
    loss.backward()
    with torch.no_grad():
        assert torch.equal(model(rgb, x), outs[0])
    blob = {"meta": np.array(repr(c)), "keys": np.array(sorted(model.state_dict().keys())),
            "x_last": outs[0].detach().numpy(), "label": label.numpy().astype(np.int16),
            "loss": np.array(loss.item()), "terms": np.array([t.item() for t in terms])}
    for i in range(3):
        blob[f"aux{i}_digest"] = digest(outs[1 + i])
        blob[f"aux{i}_s4"] = outs[1 + i].detach()[:, :, ::4, ::4].contiguous().numpy()
        blob[f"coarse{i}"] = coarse[i].numpy()
    gnames, gdig = [], []
    for n, p in model.named_parameters():
        gnames.append(n)
        gdig.append(digest(p.grad) if p.grad is not None else np.full(3, np.nan))
    blob["grad_names"] = np.array(gnames)
    blob["grad_digest"] = np.stack(gdig)
    full = [n for n, p in model.named_parameters() if ".norm_ds." in n or ".output_ds." in n]
    blob["grad_full_names"] = np.array(full)
    named = dict(model.named_parameters())
    for i, n in enumerate(full):
        blob[f"grad_full_{i}"] = named[n].grad.detach().numpy()
    path = os.path.join(HERE, f"model_{c['name']}.npz")
    np.savez_compressed(path, **blob)
    print(path, "loss %.6f" % loss.item(), "terms", [round(t.item(), 6) for t in terms], "%.0f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
