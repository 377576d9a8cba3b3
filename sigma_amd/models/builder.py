"""``EncoderDecoder`` -- drop-in boundary #1.

Mirror of /root/reference/models/builder.py:13-166 for the Sigma configurations
(``cfg.backbone`` in {sigma_tiny, sigma_small, sigma_base}, ``cfg.decoder == 'MambaDecoder'``):
same constructor signature, same attributes (``backbone``, ``decode_head``, ``criterion``,
``deep_supervision``), same ``forward(rgb, modal_x, label=None)`` contract (loss when a label
is given, logits (B, num_classes, H, W) otherwise) and the same state_dict keys.
``cfg.deep_supervision`` (absent from the reference's configs, so False) switches on the branch the reference has complete
but never selects (builder.py:102, :141-144, :158-166): three auxiliary heads in the decoder and a four-term loss.
Other backbones / decoders of the reference (SegFormer, Swin, UPerNet, ...) are other model
families and out of this path's scope; asking for them raises.
"""
from __future__ import annotations

import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

logger = logging.getLogger("sigma_amd")

_BACKBONES = {
    "sigma_tiny": ("vssm_tiny", [96, 192, 384, 768]),
    "sigma_small": ("vssm_small", [96, 192, 384, 768]),
    "sigma_base": ("vssm_base", [128, 256, 512, 1024]),
}


def _init_decoder_weights(module: nn.Module, norm_layer, bn_eps, bn_momentum):
    """utils/init_func.py:10-29 as called from builder.py:120-122: kaiming-normal (fan_in, relu)
    on every conv of the decode head; `norm_layer` instances (BatchNorm in the reference's
    train.py -- none exist in the Mamba decoder) get eps/momentum and (1, 0)."""
    for m in module.modules():
        if isinstance(m, (nn.Conv1d, nn.Conv2d, nn.Conv3d)):
            nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu")
        elif isinstance(m, norm_layer):
            m.eps = bn_eps
            m.momentum = bn_momentum
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)


class EncoderDecoder(nn.Module):
    def __init__(self, cfg=None, criterion=nn.CrossEntropyLoss(reduction="mean", ignore_index=255),
                 norm_layer=nn.BatchNorm2d):
        super().__init__()
        # The committed solution table for the remaining vendor GEMMs (sigma_amd/tuning.py) switches PyTorch's TunableOp
        # on PROCESS-WIDE: constructing a model does not do that behind the caller's back.  Entry points call
        # sigma_amd.tuning.enable_tuned_gemms() themselves (bench.py, tools/); an unchanged train.py opts in with
        # SIGMA_TUNED_GEMMS=1 in its environment.
        import os
        if os.environ.get("SIGMA_TUNED_GEMMS") == "1":
            from ..tuning import enable_tuned_gemms
            enable_tuned_gemms()
        else:
            from ..tuning import table_path, tuned_gemms_requested
            if os.path.exists(table_path()) and not tuned_gemms_requested() and not getattr(EncoderDecoder, "_tuning_note", False):
                EncoderDecoder._tuning_note = True           # once per process
                logger.info("sigma_amd: the tuned vendor-GEMM table %s is NOT in use (a few per cent of the step): set "
                            "SIGMA_TUNED_GEMMS=1 or call sigma_amd.tuning.enable_tuned_gemms() before training", table_path())
        self.norm_layer = norm_layer
        if cfg.backbone not in _BACKBONES:
            raise NotImplementedError(
                f"backbone {cfg.backbone!r}: only the Sigma (VMamba) backbones {sorted(_BACKBONES)} are on this path")
        name, self.channels = _BACKBONES[cfg.backbone]
        logger.info("Using backbone: V-MAMBA (%s)", cfg.backbone)
        from .encoders import dual_vmamba
        self.backbone = getattr(dual_vmamba, name)()
        self.aux_head = None
        if cfg.decoder != "MambaDecoder":
            raise NotImplementedError("only cfg.decoder == 'MambaDecoder' is a live configuration of the reference "
                                      "(every other decoder hits the deep_supervision AttributeError, builder.py:131)")
        logger.info("Using Mamba Decoder")
        from .decoders.MambaDecoder import MambaDecoder
        self.deep_supervision = bool(getattr(cfg, "deep_supervision", False))
        if self.deep_supervision:
            self._check_deep_size(cfg.image_height, cfg.image_width)
        self.decode_head = MambaDecoder(img_size=[cfg.image_height, cfg.image_width], in_channels=self.channels,
                                        num_classes=cfg.num_classes, embed_dim=self.channels[0],
                                        deep_supervision=self.deep_supervision)
        self.criterion = criterion
        if self.criterion:
            self.init_weights(cfg, pretrained=getattr(cfg, "pretrained_model", None))
        # nn.Linear GEMMs: hand-written split-operand bf16 MFMA kernels (sigma_amd/gemm.py, csrc/gemm_split.hip);
        # SIGMA_GEMM=fp32 keeps the vendor fp32 GEMMs
        from ..gemm import enable_split3_linears, gemm_mode
        self.gemm_mode = gemm_mode()
        self.split_linears = 0
        if self.gemm_mode == "split3":
            self.split_linears = enable_split3_linears(self)

    def init_weights(self, cfg, pretrained=None):
        if pretrained:
            # builder.py:110-114 calls backbone.init_weights, which the Sigma backbone does not define
            raise AttributeError("cfg.pretrained_model must stay None for Sigma backbones (configs/*: 'do not need to change')")
        logger.info("Initing weights ...")
        _init_decoder_weights(self.decode_head, self.norm_layer, cfg.bn_eps, cfg.bn_momentum)

    @staticmethod
    def _check_deep_size(height, width):
        """the aux branch of the reference (MambaDecoder.py:242-257) has no resize to the skip size: every stage must halve
        exactly, down to 1 / 32"""
        if height % 32 != 0 or width % 32 != 0:
            raise ValueError(f"deep_supervision needs an image height and width that are multiples of 32, got {height}x{width}")

    def encode_decode(self, rgb, modal_x):
        """backbone -> decoder -> bilinear resize to the input size (builder.py:128-144); with deep supervision the
        decoder's 4-tuple (x_last, x_output_0, x_output_1, x_output_2) as it is (builder.py:141-144)."""
        if self.deep_supervision:
            self._check_deep_size(rgb.shape[2], rgb.shape[3])
            return self.decode_head(self.backbone(rgb, modal_x))
        feats = self.backbone(rgb, modal_x)
        out = self.decode_head(feats)
        if tuple(out.shape[2:]) == tuple(rgb.shape[2:]):
            # builder.py:135 resizes to the input size; the Mamba decoder already delivers it, and a bilinear resize to the
            # same size (align_corners=False) is the identity (source index == destination index, weight 1): skipped
            return out
        return F.interpolate(out, size=rgb.shape[2:], mode="bilinear", align_corners=False)

    def _forward_deep(self, rgb, modal_x, label):
        """builder.py:158-166: criterion(x_last) + sum of criterion(x_output_i), every term against the unscaled label.  An
        aux term takes the fused upsample + loss kernels where they apply (pointwise.upsampled_cross_entropy: the plain
        criterion; pointwise.upsampled_loss: weights, smoothing, 'sum' / 'none', FocalLoss2d, ProbOhemCrossEntropy2d; up to 64
        classes), else the expansion of its coarse logits and the route of the main logits.  Without a
        label: x_last alone, the aux heads are not run."""
        self._check_deep_size(rgb.shape[2], rgb.shape[3])
        head = self.decode_head
        feats = self.backbone(rgb, modal_x)
        if label is None:
            out = head.up_x4(head.forward_up_features(feats), head.patch_size)
            return out if out.is_contiguous() else out.contiguous()
        from ..pointwise import upsampled_cross_entropy, upsampled_loss
        from .decoders.MambaDecoder import expand_logits
        x_last, aux = head.forward_deep(feats)
        loss = self._loss(x_last, label)
        for z, s in aux:
            term = upsampled_cross_entropy(self.criterion, z, s, label) if z.is_cuda else None
            if term is None and z.is_cuda:
                term = upsampled_loss(self.criterion, z, s, label)
            loss = loss + (term if term is not None else self._loss(expand_logits(z, s), label))
        return loss

    def attach_teacher(self, teacher, criterion):
        """Distillation: from here on ``forward(rgb, modal_x, label)`` returns ``criterion(student logits, label, teacher
        logits)`` (a ``DistillLoss2d``) with the teacher run under no_grad on the same batch; ``self.criterion`` is not used on
        that path and nothing else changes.  The teacher -- an ``EncoderDecoder`` of the same class count on the same device --
        is put in eval(), its parameters are frozen, and it is held UNREGISTERED: it is not in parameters(), state_dict() or
        modules(), and train() and to() do not touch it, so optimizers, checkpoints and DDP see the student alone."""
        if getattr(self, "deep_supervision", False):
            raise ValueError("attach_teacher: a student with deep_supervision is not supported (there is no fused upsample + "
                             "distillation loss for the auxiliary heads)")
        nc, nc_t = self.decode_head.num_classes, teacher.decode_head.num_classes
        if nc_t != nc:
            raise ValueError(f"attach_teacher: the teacher has {nc_t} classes, the student {nc}")
        dev, dev_t = next(self.parameters()).device, next(teacher.parameters()).device
        if dev_t != dev:
            raise ValueError(f"attach_teacher: the teacher is on {dev_t}, the student on {dev}")
        teacher.eval()
        teacher.requires_grad_(False)
        self._distill = (teacher, criterion)           # a tuple: nn.Module registers nothing inside it

    def detach_teacher(self):
        """forward is again what it was before ``attach_teacher``"""
        self._distill = None

    def forward(self, rgb, modal_x, label=None):
        distill = getattr(self, "_distill", None)
        if distill is not None and label is not None:
            teacher, criterion = distill
            with torch.no_grad():
                # the logits as the classifier lays them out (channels-last rows): forward() would re-lay them as (B, nc, H, W)
                t = teacher(rgb, modal_x) if getattr(teacher, "deep_supervision", False) else teacher.encode_decode(rgb, modal_x)
            return criterion(self.encode_decode(rgb, modal_x), label, t)
        if getattr(self, "deep_supervision", False):
            return self._forward_deep(rgb, modal_x, label)
        out = self.encode_decode(rgb, modal_x)
        if label is not None:
            return self._loss(out, label)
        return out if out.is_contiguous() else out.contiguous()     # callers get the reference's (B, nc, H, W) layout

    def _loss(self, out, label):
        """criterion(out, label) for (B, nc, H, W) logits"""
        # cross entropy (any weight / label_smoothing / reduction; 'none' gives (B, H, W)) straight from the channels-last
        # logits of the classifier GEMM (csrc/pointwise.hip); any other criterion / layout: the criterion itself on the
        # (B, nc, H, W) view
        from ..pointwise import cross_entropy, cross_entropy_deterministic
        loss = cross_entropy(self.criterion, out, label) if out.is_cuda else None
        if loss is None and torch.are_deterministic_algorithms_enabled():
            # deterministic mode: torch's nll_loss2d has no deterministic form (sigma_amd/deterministic.py)
            loss = cross_entropy_deterministic(self.criterion, out, label)
        return loss if loss is not None else self.criterion(out, label.long())
