"""The product model with deep supervision switched on, for tests/test_deepsup_cpu.py and tests/test_deepsup_gpu.py."""
import os

import torch

from tests.model_utils import cfg_for, fill


def build_ds_model(num_classes=9, H=64, W=96, criterion=None):
    """tests/model_utils.build_model with ``cfg.deep_supervision = True``: parameters from tests/golden/fill.py"""
    from sigma_amd.models.builder import EncoderDecoder
    cfg = cfg_for("sigma_tiny", num_classes, H, W)
    cfg.deep_supervision = True
    crit = criterion if criterion is not None else torch.nn.CrossEntropyLoss(reduction="mean", ignore_index=255)
    cwd = os.getcwd()
    os.chdir("/tmp")                  # the (absent) pretrained/ path is relative, as in the reference
    try:
        model = EncoderDecoder(cfg, criterion=crit, norm_layer=torch.nn.BatchNorm2d)
    finally:
        os.chdir(cwd)
    fill.fill_parameters(model)
    return model
