"""The five blocks of the model, built from the product's kernels and autograd Functions, against their fp64 twins
(tests/block_fp64_twin.py) on every branch the host code chooses; run with -m gpu.  DESIGN.md 4.7a.

Per case: the product block (default configuration, seeded non-trivial weights from tests/golden/fill.py,
``gemm.enable_split3_linears`` as ``build_model`` applies it) runs forward + backward with a seeded output gradient under
``recording()``; the float64 twin runs on the same device with the same weights, inputs and -- in training mode -- the
same per-sample stochastic-depth factors (the generator is re-seeded and the masks are drawn in the product's order).
Every output, input gradient and parameter gradient is compared slice by slice:

    err(slice) = ||got - ref64|| / ||ref64||  <=  bound(slice) = 2 (e32 + e_pert) + 2^-23

with e32 the float32 twin and e_pert the float64 twin whose every matrix product is as wrong as a two-piece GEMM may be
(largest of three seeds), both against the clean float64 twin on the case's own data.  No constant is fitted to what the
kernels achieve.  A slice whose reference is exactly zero (every parameter gradient of a dropped sample's branch, ...)
must be exactly zero.

Branches.  Every recorded launch key is reduced to the fields a host branch controls (``reduce_key``); each case asserts
the reduced keys written out in KEYS with the number of launches of each (the x_proj and dt_proj GEMMs share one reduced
key, so the set alone would not see dt_proj move to the vendor's GEMM): a silent change of branch fails the case.  The
last test asserts that every reduced key sigma_small 480x640 and sigma_base 720x1280 meet is met by some block case,
except the keys of OUTSIDE: the launches of the model's parts that are none of the five blocks.
"""
from __future__ import annotations

import collections
import functools
import importlib
import math
import time

import pytest
import torch

from tests import block_fp64_twin as twin
from tests.model_utils import fill
from tests.test_stream_fp64_gpu import CENSUS_MODELS, _census, recording

pytestmark = pytest.mark.gpu

DEV = "cuda"
DROP = 0.4


# ---------------------------------------------------------------------------------------------------------------------
# cases: id -> (kind, (B, H, W, C), d_state, mode); mode "eval" | "train" (drop_path = 0.4, masks drawn) | "plain"
# (training mode without stochastic depth, as the first blocks of an encoder stage run)

CASES = {
    # SS2D / VSSBlock: the branches of SS2D.forward and SS2DCoreFn (sigma_amd/ss2d_fused.py: legal, short, mid, R % 4)
    "vss-L96": ("vss", (2, 8, 12, 64), 16, "plain"),        # every projection on our kernels, linear_xz
    "vss-L640": ("vss", (2, 16, 40, 64), 16, "plain"),      # dw off, row-lane scan
    "vss-L1232": ("vss", (1, 28, 44, 64), 16, "plain"),     # only xd; vendor dt_proj.  Batch 1: the twin's scan dominates
    "vss-R6": ("vss", (2, 8, 12, 96), 16, "plain"),         # own_dt and dw off
    "vss-c-odd": ("vss", (2, 8, 12, 48), 4, "plain"),       # R + 2N odd: every projection vendor, _pair_sum_add
    "vss-L63": ("vss", (2, 7, 9, 64), 16, "plain"),         # M % 4 != 0: split_xz + gradient-buffer hand-off, legal false
    "vss-d512": ("vss", (1, 8, 12, 256), 16, "plain"),      # d = 512: in_proj's input gradient cuts its reduction into slices
    "vss-L96-train": ("vss", (6, 8, 12, 64), 16, "train"),  # mask in the gated LayerNorm, residual in the out_proj GEMM
    "vss-L96-eval": ("vss", (2, 8, 12, 64), 16, "eval"),
    "cromb-64-eval": ("cromb", (2, 8, 12, 64), 4, "eval"),
    "cromb-64-train": ("cromb", (2, 8, 12, 64), 4, "train"),
    "cromb-96-eval": ("cromb", (2, 7, 9, 96), 4, "eval"),
    "cromb-96-train": ("cromb", (2, 7, 9, 96), 4, "train"),
    "conmb-64-eval": ("conmb", (2, 8, 12, 64), 4, "eval"),
    "conmb-64-train": ("conmb", (2, 8, 12, 64), 4, "train"),
    "conmb-96-eval": ("conmb", (1, 7, 9, 96), 4, "eval"),
    "conmb-96-train": ("conmb", (1, 7, 9, 96), 4, "train"),
    "cvss-96-eval": ("cvss", (2, 8, 12, 96), 4, "eval"),
    "cvss-96-train": ("cvss", (2, 8, 12, 96), 4, "train"),
    "cvss-64-eval": ("cvss", (1, 7, 9, 64), 4, "eval"),
    "cvss-64-train": ("cvss", (1, 7, 9, 64), 4, "train"),
    "merge-odd": ("merge", (2, 7, 9, 64), 0, "eval"),
    "merge-even": ("merge", (2, 8, 12, 96), 0, "eval"),
}

N_MASKS = {"vss": 1, "cvss": 1, "cromb": 2, "conmb": 1, "merge": 0}


def reduce_key(k):
    """a launch key of tests/test_stream_fp64_gpu.py::launch_key cut down to what a host branch of the blocks controls:
    GEMM (form, pieces, batched, a_mod, shared output, k_slices, t_cols, residuals, bias, accumulate, stage);
    LayerNorm (direction, gate, row_scale, dx_add); dwconv (direction, n_orders, strided, deterministic bit);
    scan (direction); every other launch its symbol"""
    if k[0] == "gemm":
        return k[:11] + (k[13],)
    if k[0] in ("ln_fwd", "ln_bwd", "dw_fwd", "dw_bwd"):
        return (k[0],) + tuple(k[2:])
    return (k[0],)


# ---------------------------------------------------------------------------------------------------------------------
# expected reduced keys

def _g(form, pieces=2, batched=False, a_mod=False, shared=False, k_slices=False, t_cols=False, res=0, bias=False, acc=False,
       stage="own"):
    return ("gemm", form, pieces, batched, a_mod, shared, k_slices, t_cols, res, bias, acc, stage)


KEYS: dict = {}
for _cid in ('vss-L96', 'vss-L96-eval'):
    KEYS[_cid] = {
        ('dw_bwd', 2, True, False): 1,
        ('dw_fwd', 2, True): 1,
        _g('nn'): 2,
        _g('nn', k_slices=True): 1,
        _g('nn', batched=True, a_mod=True): 2,
        _g('nn', batched=True, a_mod=True, res=2): 1,
        _g('nt', res=1): 1,
        _g('nt', t_cols=True): 1,
        _g('nt', batched=True, shared=True, stage='two-stage'): 2,
        _g('tn'): 2,
        _g('tn', acc=True): 1,
        ('ln_bwd', False, False, True): 1,
        ('ln_bwd', True, False, False): 1,
        ('ln_fwd', False, False): 1,
        ('ln_fwd', True, False): 1,
        ('merge',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
    }
for _cid in ('vss-L640',):
    KEYS[_cid] = {
        ('dw_bwd', 2, True, False): 1,
        ('dw_fwd', 2, True): 1,
        _g('nn'): 2,
        _g('nn', k_slices=True, stage='two-stage'): 1,
        _g('nn', batched=True, a_mod=True): 2,
        _g('nn', batched=True, a_mod=True, res=2): 1,
        _g('nt', res=1): 1,
        _g('nt', t_cols=True): 1,
        _g('nt', batched=True, shared=True, stage='two-stage'): 1,
        _g('tn', stage='two-stage'): 2,
        _g('tn', acc=True): 1,
        ('ln_bwd', False, False, True): 1,
        ('ln_bwd', True, False, False): 1,
        ('ln_fwd', False, False): 1,
        ('ln_fwd', True, False): 1,
        ('merge',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
    }
for _cid in ('vss-L1232',):
    KEYS[_cid] = {
        ('dw_bwd', 2, True, False): 1,
        ('dw_fwd', 2, True): 1,
        _g('nn'): 2,
        _g('nn', k_slices=True, stage='two-stage'): 1,
        _g('nn', batched=True): 1,
        _g('nn', batched=True, res=2): 1,
        _g('nt', res=1): 1,
        _g('nt', t_cols=True): 1,
        _g('tn', stage='two-stage'): 2,
        _g('tn', acc=True): 1,
        ('ln_bwd', False, False, True): 1,
        ('ln_bwd', True, False, False): 1,
        ('ln_fwd', False, False): 1,
        ('ln_fwd', True, False): 1,
        ('merge',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
    }
for _cid in ('vss-R6',):
    KEYS[_cid] = {
        ('dw_bwd', 2, True, False): 1,
        ('dw_fwd', 2, True): 1,
        _g('nn'): 2,
        _g('nn', k_slices=True): 1,
        _g('nn', batched=True, a_mod=True): 1,
        _g('nn', batched=True, a_mod=True, res=2): 1,
        _g('nt', res=1): 1,
        _g('nt', t_cols=True): 1,
        _g('nt', batched=True, shared=True, stage='two-stage'): 1,
        _g('tn'): 2,
        _g('tn', acc=True): 1,
        ('ln_bwd', False, False, True): 1,
        ('ln_bwd', True, False, False): 1,
        ('ln_fwd', False, False): 1,
        ('ln_fwd', True, False): 1,
        ('merge',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
    }
for _cid in ('vss-c-odd',):
    KEYS[_cid] = {
        ('dw_bwd', 2, True, False): 1,
        ('dw_fwd', 2, True): 1,
        _g('nn'): 2,
        _g('nn', k_slices=True): 1,
        _g('nt', res=1): 1,
        _g('nt', t_cols=True): 1,
        _g('tn'): 2,
        _g('tn', acc=True): 1,
        ('ln_bwd', False, False, True): 1,
        ('ln_bwd', True, False, False): 1,
        ('ln_fwd', False, False): 1,
        ('ln_fwd', True, False): 1,
        ('merge',): 1,
        ('pair_sum_add',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
    }
for _cid in ('vss-L63',):
    KEYS[_cid] = {
        ('dw_bwd', 2, False, False): 1,
        ('dw_fwd', 2, False): 1,
        _g('nn'): 2,
        _g('nt'): 1,
        _g('nt', res=1): 1,
        _g('tn'): 2,
        ('ln_bwd', False, False, True): 1,
        ('ln_bwd', True, False, False): 1,
        ('ln_fwd', False, False): 1,
        ('ln_fwd', True, False): 1,
        ('merge',): 1,
        ('pair_sum_add',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
        ('transpose',): 2,
    }
for _cid in ('vss-d512',):
    KEYS[_cid] = {
        ('dw_bwd', 2, True, False): 1,
        ('dw_fwd', 2, True): 1,
        _g('nn'): 2,
        _g('nn', k_slices=True): 1,
        _g('nn', batched=True): 2,
        _g('nn', batched=True, res=2): 1,
        _g('nt', res=1): 1,
        _g('nt', t_cols=True): 1,
        _g('nt', batched=True): 2,
        _g('tn'): 2,
        _g('tn', acc=True, stage='two-stage'): 1,
        ('ln_bwd', False, False, True): 1,
        ('ln_bwd', True, False, False): 1,
        ('ln_fwd', False, False): 1,
        ('ln_fwd', True, False): 1,
        ('merge',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
    }
for _cid in ('vss-L96-train',):
    KEYS[_cid] = {
        ('dw_bwd', 2, True, False): 1,
        ('dw_fwd', 2, True): 1,
        _g('nn'): 2,
        _g('nn', k_slices=True, stage='two-stage'): 1,
        _g('nn', batched=True, a_mod=True): 2,
        _g('nn', batched=True, a_mod=True, res=2): 1,
        _g('nt', res=1): 1,
        _g('nt', t_cols=True): 1,
        _g('nt', batched=True, shared=True, stage='two-stage'): 2,
        _g('tn', stage='two-stage'): 2,
        _g('tn', acc=True): 1,
        ('ln_bwd', False, False, True): 1,
        ('ln_bwd', True, True, False): 1,
        ('ln_fwd', False, False): 1,
        ('ln_fwd', True, True): 1,
        ('merge',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
    }
for _cid in ('cromb-64-eval', 'cromb-64-train', 'cromb-96-eval', 'cromb-96-train'):
    KEYS[_cid] = {
        ('dw_bwd', 1, False, False): 1,
        ('dw_fwd', 1, False): 1,
        _g('nn'): 4,
        _g('nt'): 4,
        _g('tn'): 4,
        ('ln_bwd', False, False, False): 2,
        ('ln_fwd', False, False): 2,
        ('scan_bwd',): 2,
        ('scan_fwd',): 2,
        ('transpose',): 8,
    }
for _cid in ('conmb-64-eval', 'conmb-64-train', 'conmb-96-eval', 'conmb-96-train'):
    KEYS[_cid] = {
        ('dw_bwd', 1, False, False): 2,
        ('dw_fwd', 1, False): 2,
        _g('nn'): 3,
        _g('nt'): 3,
        _g('tn'): 3,
        ('ln_bwd', False, False, False): 2,
        ('ln_fwd', False, False): 2,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('transpose',): 8,
    }
for _cid in ('cvss-96-eval',):
    KEYS[_cid] = {
        ('colscale_bwd',): 2,
        ('dw_bwd', 2, True, False): 1,
        ('dw_fwd', 2, True): 1,
        _g('nn'): 2,
        _g('nn', k_slices=True): 1,
        _g('nn', batched=True, a_mod=True): 1,
        _g('nn', batched=True, a_mod=True, res=2): 1,
        _g('nt'): 1,
        _g('nt', t_cols=True): 1,
        _g('nt', batched=True, shared=True, stage='two-stage'): 1,
        _g('tn'): 2,
        _g('tn', acc=True): 1,
        ('ln_bwd', False, False, True): 2,
        ('ln_bwd', True, False, False): 1,
        ('ln_fwd', False, False): 2,
        ('ln_fwd', True, False): 1,
        ('merge',): 1,
        ('plane_dot',): 1,
        ('plane_gate_bwd',): 1,
        ('plane_pool',): 1,
        ('plane_scale',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
        ('transpose',): 4,
    }
for _cid in ('cvss-96-train',):
    KEYS[_cid] = {
        ('colscale_bwd',): 2,
        ('dw_bwd', 2, True, False): 1,
        ('dw_fwd', 2, True): 1,
        _g('nn'): 2,
        _g('nn', k_slices=True): 1,
        _g('nn', batched=True, a_mod=True): 1,
        _g('nn', batched=True, a_mod=True, res=2): 1,
        _g('nt'): 1,
        _g('nt', t_cols=True): 1,
        _g('nt', batched=True, shared=True, stage='two-stage'): 1,
        _g('tn'): 2,
        _g('tn', acc=True): 1,
        ('ln_bwd', False, False, True): 2,
        ('ln_bwd', True, True, False): 1,
        ('ln_fwd', False, False): 2,
        ('ln_fwd', True, True): 1,
        ('merge',): 1,
        ('plane_dot',): 1,
        ('plane_gate_bwd',): 1,
        ('plane_pool',): 1,
        ('plane_scale',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
        ('transpose',): 4,
    }
for _cid in ('cvss-64-eval',):
    KEYS[_cid] = {
        ('colscale_bwd',): 2,
        ('dw_bwd', 2, False, False): 1,
        ('dw_fwd', 2, False): 1,
        _g('nn'): 2,
        _g('nt'): 2,
        _g('tn'): 2,
        ('ln_bwd', False, False, True): 2,
        ('ln_bwd', True, False, False): 1,
        ('ln_fwd', False, False): 2,
        ('ln_fwd', True, False): 1,
        ('merge',): 1,
        ('pair_sum_add',): 1,
        ('plane_dot',): 1,
        ('plane_gate_bwd',): 1,
        ('plane_pool',): 1,
        ('plane_scale',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
        ('transpose',): 6,
    }
for _cid in ('cvss-64-train',):
    KEYS[_cid] = {
        ('colscale_bwd',): 2,
        ('dw_bwd', 2, False, False): 1,
        ('dw_fwd', 2, False): 1,
        _g('nn'): 2,
        _g('nt'): 2,
        _g('tn'): 2,
        ('ln_bwd', False, False, True): 2,
        ('ln_bwd', True, True, False): 1,
        ('ln_fwd', False, False): 2,
        ('ln_fwd', True, True): 1,
        ('merge',): 1,
        ('pair_sum_add',): 1,
        ('plane_dot',): 1,
        ('plane_gate_bwd',): 1,
        ('plane_pool',): 1,
        ('plane_scale',): 1,
        ('scan_bwd',): 1,
        ('scan_fwd',): 1,
        ('split',): 1,
        ('transpose',): 6,
    }
for _cid in ('merge-odd', 'merge-even'):
    KEYS[_cid] = {
        _g('nn'): 1,
        _g('nt'): 1,
        _g('tn'): 1,
        ('ln_bwd', False, False, False): 1,
        ('ln_fwd', False, False): 1,
    }

# reduced keys of the two real models that belong to none of the five blocks: key -> the part of the model that
# launches it
OUTSIDE = {
    ("ce_fwd",): "the loss (softmax cross entropy)",
    ("ce_bwd",): "the loss (softmax cross entropy)",
    ("upsample",): "the decoder's bilinear x2 upsampling",
    _g("nt", bias=True): "the patch embedding's convolution as a GEMM with its bias; every Linear of the five blocks is bias-free",
}


# ---------------------------------------------------------------------------------------------------------------------
# running a case

def _vm():
    return importlib.import_module("sigma_amd.models.encoders.vmamba")


def _build(kind, C, N, drop):
    vm = _vm()
    if kind == "vss":
        blk = vm.VSSBlock(hidden_dim=C, drop_path=drop, d_state=N)
    elif kind == "cvss":
        blk = vm.CVSSDecoderBlock(hidden_dim=C, drop_path=drop, d_state=N)
    elif kind == "cromb":
        blk = vm.CrossMambaFusionBlock(hidden_dim=C, drop_path=drop, d_state=N)
    elif kind == "conmb":
        blk = vm.ConcatMambaFusionBlock(hidden_dim=C, drop_path=drop, d_state=N)
    else:
        blk = vm.PatchMerging2D(C)
    fill.fill_parameters(blk)
    from sigma_amd import gemm
    gemm.enable_split3_linears(blk)
    return blk.to(DEV)


def _draw(kind, B, keep):
    """the per-sample factors of one training-mode forward, drawn as the product's DropPath modules draw them (one
    (B, 1, 1, 1) Bernoulli tensor per module, in the order of the block's forward)"""
    out = []
    for _ in range(N_MASKS[kind]):
        m = torch.empty((B, 1, 1, 1), device=DEV).bernoulli_(keep)
        out.append((m / keep).flatten())
    return out


def _mask_seed(kind, B, keep):
    """the first seed whose masks drop one sample and keep one (batch 1: keep the sample; the batch-2 case of the same
    block drops one)"""
    for seed in range(256):
        torch.manual_seed(seed)
        fs = _draw(kind, B, keep)
        if all((bool((f == 0).any()) and bool((f != 0).any())) if B > 1 else bool((f != 0).all()) for f in fs):
            return seed
    raise AssertionError("no seed drops one sample and keeps one")


class CaseData:
    """what a case's runs share: the built block, its inputs and output gradients (plain tensors: every run makes its own
    leaves from them), the seed and the per-sample factors of its stochastic-depth masks, and the twin's answer on this
    data: ``ref`` (float64), ``e32``, ``e_pert`` and ``bnd`` = twin.bound(e32, e_pert) (+ EXTRA)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def _block(cid):
    kind, (B, H, W, C), N, mode = CASES[cid]
    blk = _build(kind, C, N, DROP if mode == "train" else 0.0)
    blk.train(mode != "eval")
    return blk


@functools.lru_cache(maxsize=None)
def case_data(cid, variant="base"):
    """CaseData of case ``cid``, computed once and shared by every test of the case (tests/test_autograd_contract_gpu.py
    runs the product again on it under other autograd configurations: the twin's gradient of a trainable leaf does not
    depend on which other leaves are frozen).  ``variant``: "base" the case's own data; "second" other inputs and output
    gradients for the same block (a second micro-batch); "ones" the base inputs with output gradients of ones (what
    ``out.sum().backward()`` delivers)."""
    kind, (B, H, W, C), N, mode = CASES[cid]
    t0 = time.time()
    blk = _block(cid)
    g = torch.Generator().manual_seed(1000 + sum(map(ord, cid)) + (7919 if variant == "second" else 0))
    n_in = 2 if kind in ("cromb", "conmb") else 1
    n_out = 2 if kind == "cromb" else 1
    oshape = (B, (H + 1) // 2, (W + 1) // 2, 2 * C) if kind == "merge" else (B, H, W, C)
    xs = [torch.randn(B, H, W, C, generator=g).to(DEV) for _ in range(n_in)]
    gys = [torch.randn(oshape, generator=g).to(DEV) for _ in range(n_out)]
    if variant == "ones":
        gys = [torch.ones_like(t) for t in gys]
    factors = seed = None
    if mode == "train":
        seed = _mask_seed(kind, B, 1.0 - DROP)
        torch.manual_seed(seed)
        factors = _draw(kind, B, 1.0 - DROP)
        if B > 1:
            assert all(bool((f == 0).any()) and bool((f != 0).any()) for f in factors), factors
    sd = {n: p.detach() for n, p in blk.named_parameters()}
    ref, e32, e_pert = twin.twin_reference(kind, sd, xs, gys, factors, device=DEV)
    bnd = twin.bound(e32, e_pert)
    for name, b in EXTRA.get(cid, {}).items():
        bnd[name] += b
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return CaseData(cid=cid, kind=kind, blk=blk, xs=xs, gys=gys, factors=factors, seed=seed, ref=ref, e32=e32, e_pert=e_pert,
                    bnd=bnd, twin_seconds=time.time() - t0)


def product_run(data, xs=None, frozen=None, freeze_inputs=False, log=None):
    """one forward of the product block of ``data`` on fresh leaves: (outs, leaves xs).  Parameters named by ``frozen``
    (a predicate on the name; None: none) and, with ``freeze_inputs``, the inputs do not require a gradient; every
    ``.grad`` of the block is cleared first.  Training-mode cases draw their masks from the case's seed."""
    blk = data.blk
    for n, p in blk.named_parameters():
        p.requires_grad_(not (frozen is not None and frozen(n)))
        p.grad = None
    xs = [x.detach().clone().requires_grad_(not freeze_inputs) for x in (data.xs if xs is None else xs)]
    if data.seed is not None:
        torch.manual_seed(data.seed)
    outs = blk(*xs)
    return (outs if isinstance(outs, tuple) else (outs,)), xs


def collect(data, outs, xs, missing="zeros"):
    """{"out<i>", "dx<i>", <parameter name>: gradient} of a finished run; a leaf without a gradient gives zeros
    (``missing="zeros"``: the all-trainable contract, where only an unused parameter has none) or is left out"""
    got = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    for i, x in enumerate(xs):
        if x.grad is not None or missing == "zeros":
            got[f"dx{i}"] = x.grad
    for n, p in data.blk.named_parameters():
        if p.grad is not None:
            got[n] = p.grad
        elif missing == "zeros":
            got[n] = torch.zeros_like(p)
    return got


@functools.lru_cache(maxsize=None)
def case_result(cid):
    """(ratios {slice: (err, bound)}, {reduced launch key: launches}, seconds) of case ``cid``; computed once, shared by the case's
    test and the census"""
    kind = CASES[cid][0]
    t0 = time.time()
    data = case_data(cid)
    with recording() as log:
        outs, xs = product_run(data)
        torch.autograd.backward(outs, data.gys)
        torch.cuda.synchronize()
    keys = dict(collections.Counter(reduce_key(k) for k in log if k is not None))
    got = collect(data, outs, xs)
    assert sorted(data.ref) == sorted(got)
    err = twin.slice_errors(kind, got, data.ref)
    bnd = data.bnd
    torch.cuda.synchronize()
    for p in data.blk.parameters():
        p.grad = None
    del got, outs
    return {k: (err[k], bnd[k]) for k in err}, keys, time.time() - t0


# the one exception DESIGN.md 4.7a allows: a slice that is a pure kernel reduction whose kernel passes its own fp64 test
# may add that test's companion term K u S / ||ref||.  case -> {slice: term}.  None was needed.
EXTRA: dict = {}

WORST: dict = {}


def _fmt(keys):
    return "{\n" + "".join(f"        {k!r}: {n},\n" for k, n in sorted(keys.items(), key=repr)) + "    }"


@pytest.mark.parametrize("cid", list(CASES))
def test_block_against_fp64_twin(cid):
    kind = CASES[cid][0]
    ratios, keys, secs = case_result(cid)
    print(f"\n{cid}: {secs:.1f} s, {len(ratios)} slices")
    bad = {}
    for k in sorted(ratios):
        e, b = ratios[k]
        r = e / b if b > 0 and math.isfinite(e) else (0.0 if e == 0.0 else math.inf)
        print(f"  {cid} {k:46s} err {e:.3g}  bound {b:.3g}  ratio {r:.3g}")
        if r > WORST.get(kind, (0.0, ""))[0]:
            WORST[kind] = (r, f"{cid} {k}")
        if not e <= b:
            bad[k] = (e, b)
    print(f'    "{cid}": {_fmt(keys)},')
    assert not bad, f"{cid}: slices outside the bound (err, bound): {bad}"
    want = KEYS[cid]
    diff = {k: (keys.get(k, 0), want.get(k, 0)) for k in set(keys) | set(want) if keys.get(k, 0) != want.get(k, 0)}
    assert not diff, f"{cid}: launches changed branch, key: (launched, expected) {diff}"


def test_every_branch_of_the_real_models_is_met_by_a_block_case():
    """the reduced keys of one forward + backward of both census models are a subset of the block cases' keys and
    OUTSIDE"""
    met = {}
    for cid in CASES:
        for k in case_result(cid)[1]:
            met.setdefault(k, cid)
    missing = []
    with recording() as log:
        for name, H, W, batch, classes in CENSUS_MODELS:
            seen = sorted({reduce_key(k) for k in _census(name, H, W, batch, classes, log)}, key=repr)
            print(f"\nblock census {name}: {len(seen)} reduced keys")
            for k in seen:
                where = met.get(k) or ("outside the blocks: " + OUTSIDE[k] if k in OUTSIDE else "NOT MET")
                print("  ", k, "->", where)
                if k not in met and k not in OUTSIDE:
                    missing.append((name, k))
    assert not missing, f"branches of the real models that no block case reaches: {missing}"


def test_zz_report_worst_ratios():
    """prints the worst err / bound of each block (the cases above asserted <= 1); DESIGN.md 4.7a quotes them"""
    for cid in CASES:
        kind = CASES[cid][0]
        for k, (e, b) in case_result(cid)[0].items():
            r = e / b if b > 0 and math.isfinite(e) else (0.0 if e == 0.0 else math.inf)
            if r > WORST.get(kind, (0.0, ""))[0]:
                WORST[kind] = (r, f"{cid} {k}")
    print("\nworst err / bound per block:")
    for kind, (r, where) in sorted(WORST.items()):
        print(f"   {kind:6s} {r:.3g}   {where}")
