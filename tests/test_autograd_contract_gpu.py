"""The layer between the kernels and the user -- the autograd Functions and the host code that picks them -- under the
autograd configurations every other test leaves out: frozen leaves, no-grad forwards, a second backward into existing
``.grad``s, two graphs in flight, output gradients that are not fresh contiguous tensors; run with -m gpu.  DESIGN.md 4.7b.

Block level.  The cases, blocks, data and float64 twins are those of tests/test_blocks_fp64_gpu.py (``case_data``: the
twin's gradient of a trainable leaf does not depend on which other leaves are frozen, so one reference per case serves
every pattern) and so is the bound, ``twin.bound(e32, e_pert)`` of the case: no constant of this file enters a comparison.

    pattern      frozen                                             reaches
    inputs       the block inputs                                   forward_with_pass declining, needs_input_grad[0] false,
                                                                    a no-grad residual in the out_proj GEMM
    params       every parameter                                    every dw / db branch skipped
    raw          what train_step.group_weight puts in no group      what the reference's optimizer never steps
    grouped      the complement of raw                              Linear / conv / norm frozen, raw Mamba parameters trainable
    none-nograd  nothing; forward under no_grad / inference_mode    need_x=False, NULL mean / rstd

Per (case, pattern): frozen leaves have no ``.grad``, trainable ones do; every output and trainable-gradient slice is
inside the case's bound; the recorded launches are the all-trainable table KEYS[cid] minus DROPS[(cid, pattern)] (no new
key, no larger count; the one exception, LESSER, is the first LayerNorm's backward without the joined residual gradient,
held against the joined launch it replaces); under torch's deterministic flag outputs and trainable gradients equal the all-trainable run's
bit for bit.  Then, all-trainable: two backwards through one retained graph, two graphs in flight (LIFO and FIFO), and
the same output gradient delivered permuted, misaligned and as the stride-0 expansion of ``out.sum().backward()``.

Function level: the Functions with one consumer or one ``needs_input_grad`` entry at a time against fp64 torch with the
bounds of tests/test_gemm_gpu.py and tests/test_stream_fp64_gpu.py, and ``fwd_ext(need_x=False)`` for every forward
family.  Model level: tests/autograd_contract_worker.py in one child process.

The negative controls at the end run the checkers of this file on wrong references (no product code involved beyond the
results already computed).
"""
from __future__ import annotations

import collections
import contextlib
import functools
import math
import os
import subprocess
import sys
import time

import pytest
import torch

from tests import block_fp64_twin as twin
from tests.test_blocks_fp64_gpu import CASES, KEYS, _g, case_data, collect, product_run, reduce_key
from tests.test_deterministic_gpu import deterministic
from tests.test_stream_fp64_gpu import recording

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

BASE = ["vss-L96", "vss-L63", "vss-L96-train", "cromb-64-train", "conmb-64-train", "cvss-96-train", "merge-odd"]
LAYOUT = ["vss-L96", "vss-L63", "cvss-96-train", "merge-odd"]
FREEZE = ("inputs", "params", "raw", "grouped")

# Block kinds that contain a vendor convolution: CVSSDecoderBlock's ChannelAttentionBlock is two dense 3x3 nn.Conv2d
# (MIOpen).  MIOpen's dense 3x3 convolutions do not repeat bitwise from call to call outside deterministic mode
# (tests/test_model_gpu.py::test_train_mode_step_and_determinism_of_forward), so the no-grad output of these blocks is held
# to the twin's bound instead of torch.equal.  Every other convolution of the five blocks is depthwise 3x3 + SiLU on
# csrc/dwconv.hip (vmamba._conv_act, dwconv_silu_two_orders), and PatchMerging2D has none.
VENDOR_CONV = {"cvss": "ChannelAttentionBlock: conv_blk.cab.0 / cab.2 are dense 3x3 nn.Conv2d (MIOpen)"}

# Slices kept under the twin's bound instead of bitwise equality under the flag: (case, pattern, slice) -> reason.
NOT_BITWISE: dict = {}

WORST: dict = {}
SECONDS: dict = {}


@contextlib.contextmanager
def flagged():
    """torch's deterministic flag with the vendor GEMM's workspace setting it demands, both restored afterwards"""
    var = "CUBLAS_WORKSPACE_CONFIG"
    old = os.environ.get(var)
    os.environ[var] = ":4096:8"
    try:
        with deterministic():
            yield
    finally:
        if old is None:
            os.environ.pop(var, None)
        else:
            os.environ[var] = old


@contextlib.contextmanager
def timed(what):
    t0 = time.time()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        SECONDS[what] = time.time() - t0
        print(f"\n{what}: {SECONDS[what]:.2f} s")


# ---------------------------------------------------------------------------------------------------------------------
# patterns

def raw_names(blk):
    """names of the parameters train_step.group_weight(blk, lr) puts in no group"""
    from sigma_amd.train_step import group_weight
    grouped = {id(p) for g in group_weight(blk, 1e-3) for p in g["params"]}
    return {n for n, p in blk.named_parameters() if id(p) not in grouped}


def pattern_of(data, pattern):
    """(predicate on parameter names: frozen, inputs frozen)"""
    raw = raw_names(data.blk)
    if pattern == "none":
        return (lambda n: False), False
    if pattern == "inputs":
        return (lambda n: False), True
    if pattern == "params":
        return (lambda n: True), False
    if pattern == "raw":
        return (lambda n: n in raw), False
    if pattern == "grouped":
        return (lambda n: n not in raw), False
    raise KeyError(pattern)


def applies(cid, pattern):
    """raw / grouped need a block that owns raw parameters (PatchMerging2D has none: raw would freeze nothing and grouped
    would be params again)"""
    return pattern in ("inputs", "params") or CASES[cid][0] != "merge"


def trainable_names(data, pattern):
    """names of the outputs and of the leaves that must receive a gradient under ``pattern``"""
    frozen, no_inputs = pattern_of(data, pattern)
    n_in = len(data.xs)
    names = [k for k in data.ref if k.startswith("out") and "." not in k]
    if not no_inputs:
        names += [f"dx{i}" for i in range(n_in)]
    names += [n for n, _ in data.blk.named_parameters() if not frozen(n)]
    return names


def frozen_names(data, pattern):
    frozen, no_inputs = pattern_of(data, pattern)
    return ([f"dx{i}" for i in range(len(data.xs))] if no_inputs else []) + [n for n, _ in data.blk.named_parameters() if frozen(n)]


def run(data, pattern="none", gys=None, record=False, xs=None):
    """one forward + backward of the product under ``pattern``: ({name: tensor} without the frozen leaves, reduced launch
    keys or None)"""
    frozen, no_inputs = pattern_of(data, pattern)
    with (recording() if record else contextlib.nullcontext([])) as log:
        outs, leaves = product_run(data, xs=xs, frozen=frozen, freeze_inputs=no_inputs)
        torch.autograd.backward(outs, data.gys if gys is None else gys)
        torch.cuda.synchronize()
    keys = dict(collections.Counter(reduce_key(k) for k in log if k is not None)) if record else None
    got = collect(data, outs, leaves, missing="leave")
    _reset(data)
    return got, keys


def _reset(data):
    for p in data.blk.parameters():
        p.requires_grad_(True)
        p.grad = None


# ---------------------------------------------------------------------------------------------------------------------
# checkers

def ratios_against(kind, got, ref, bnd, names):
    """{slice: (err, bound)} of the tensors ``names`` of ``got`` against ``ref``.  A name the product has no tensor for
    fails: a leaf the reference calls trainable must have a gradient."""
    missing = [n for n in names if got.get(n) is None]
    assert not missing, f"no gradient for leaves the reference has one for: {missing}"
    err = twin.slice_errors(kind, got, {n: ref[n] for n in names})
    return {k: (e, bnd[k]) for k, e in err.items()}


def outside(ratios):
    return {k: (e, b) for k, (e, b) in ratios.items() if not e <= b}


def note_worst(pattern, cid, ratios):
    for k, (e, b) in ratios.items():
        r = e / b if b > 0 and math.isfinite(e) else (0.0 if e == 0.0 else math.inf)
        if r >= WORST.get(pattern, (-1.0, ""))[0]:
            WORST[pattern] = (r, f"{cid} {k}")


def unequal(a, b, names):
    """names whose tensors are not bitwise equal"""
    return [n for n in names if not torch.equal(a[n], b[n])]


def scaled(ref, s):
    return {k: v * s for k, v in ref.items()}


def sum_bound(kind, da, db, names):
    """bound of the slices of gA + gB against refA + refB, from the two cases' own bounds by the triangle inequality:
    ||(gA + gB) - (rA + rB)|| <= bA ||rA|| + bB ||rB||, relative to ||rA + rB||.  No new constant."""
    out = {}
    for n in names:
        for (label, ra), (_, rb) in zip(twin.slices(kind, n, da.ref[n].double()), twin.slices(kind, n, db.ref[n].double())):
            den = float((ra + rb).norm())
            num = da.bnd[label] * float(ra.norm()) + db.bnd[label] * float(rb.norm())
            out[label] = num / den if den > 0 else 0.0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# shared product results (each computed once)

@functools.lru_cache(maxsize=None)
def flagged_base(cid, variant="base"):
    """the all-trainable run of the case under the flag: what every pattern must reproduce bit for bit"""
    data = case_data(cid, variant)
    with flagged():
        return run(data)[0]


@functools.lru_cache(maxsize=None)
def plain_base(cid):
    """the all-trainable run without the flag, with its launches"""
    return run(case_data(cid), record=True)


# launches of the all-trainable table that a pattern does not issue: (case, pattern) -> {reduced key: launches dropped}.
# The observed table of the pair is KEYS[cid] minus this (and, for LESSER, with the launch counted under its own key).
# DESIGN.md 4.7b lists them by name.
_LN_JOINED = ("ln_bwd", False, False, True)
_XZ = {_g("nn", k_slices=True): 1, _g("tn"): 2}              # in_proj's two weight-gradient GEMMs and out_proj's
_XZ_2 = {_g("nn", k_slices=True, stage="two-stage"): 1, _g("tn", stage="two-stage"): 2}
DROPS = {
    ("vss-L96", "inputs"): {_LN_JOINED: 1},
    ("vss-L96", "params"): _XZ,
    ("vss-L96", "raw"): {},
    ("vss-L96", "grouped"): _XZ,
    ("vss-L63", "inputs"): {_LN_JOINED: 1},
    ("vss-L63", "params"): {_g("tn"): 2},
    ("vss-L63", "raw"): {},
    ("vss-L63", "grouped"): {_g("tn"): 2},
    ("vss-L96-train", "inputs"): {_LN_JOINED: 1},
    ("vss-L96-train", "params"): _XZ_2,
    ("vss-L96-train", "raw"): {},
    ("vss-L96-train", "grouped"): _XZ_2,
    ("cromb-64-train", "inputs"): {_g("nn"): 2},             # the input gradients of the two in_proj
    ("cromb-64-train", "params"): {_g("tn"): 4},
    ("cromb-64-train", "raw"): {},
    ("cromb-64-train", "grouped"): {_g("tn"): 4},
    ("conmb-64-train", "inputs"): {_g("nn"): 2},
    ("conmb-64-train", "params"): {_g("tn"): 3},
    ("conmb-64-train", "raw"): {},
    ("conmb-64-train", "grouped"): {_g("tn"): 3},
    ("cvss-96-train", "inputs"): {_LN_JOINED: 1},
    ("cvss-96-train", "params"): _XZ,
    ("cvss-96-train", "raw"): {},
    ("cvss-96-train", "grouped"): _XZ,
    ("merge-odd", "inputs"): {},
    ("merge-odd", "params"): {_g("tn"): 1},
}

# The one launch a pattern issues under a reduced key of its own: with the block input frozen, forward_with_pass declines
# and the first LayerNorm's backward runs without the residual gradient joined in its kernel (dx_add absent) -- the same
# kernel with one operand less, in place of the joined launch the all-trainable run makes.  It is counted against the
# table entry of the launch it stands for: lesser key -> the key of KEYS it is held against.
LESSER = {("ln_bwd", False, False, False): _LN_JOINED}
# (case, pattern) -> {lesser key: launches}; every other pair issues none
LESSER_LAUNCHES = {(c, "inputs"): {("ln_bwd", False, False, False): 1} for c in ("vss-L96", "vss-L63", "vss-L96-train", "cvss-96-train")}


def expected_keys(cid, pattern):
    want = dict(KEYS[cid])
    for k, n in DROPS[(cid, pattern)].items():
        want[k] = want.get(k, 0) - n
    for k, n in LESSER_LAUNCHES.get((cid, pattern), {}).items():
        want[k] = want.get(k, 0) + n
    return {k: n for k, n in want.items() if n != 0}


def held_against_the_table(keys, full):
    """{table key: (launched, all-trainable)} where a pattern launches more than the all-trainable run, a launch of
    LESSER counted under the table key it stands for (only where the table has none of its own)"""
    folded: dict = collections.Counter()
    for k, n in keys.items():
        folded[LESSER[k] if (k in LESSER and k not in full) else k] += n
    return {k: (n, full.get(k, 0)) for k, n in folded.items() if n > full.get(k, 0)}


def _fmt(d):
    return "{" + ", ".join(f"{k!r}: {n}" for k, n in sorted(d.items(), key=repr)) + "}"


# ---------------------------------------------------------------------------------------------------------------------
# freeze patterns

PAIRS = [(c, p) for c in BASE for p in FREEZE if applies(c, p)]


@pytest.mark.parametrize("cid,pattern", PAIRS, ids=[f"{c}-{p}" for c, p in PAIRS])
def test_frozen_leaves(cid, pattern):
    data = case_data(cid)
    kind = data.kind
    with timed(f"{cid} {pattern}"):
        got, keys = run(data, pattern, record=True)
        names, frozen = trainable_names(data, pattern), frozen_names(data, pattern)
        problems = []
        # frozen leaves have no gradient, trainable ones do
        have = [n for n in frozen if got.get(n) is not None]
        if have:
            problems.append(f"frozen leaves with a gradient: {have}")
        ratios = ratios_against(kind, got, data.ref, data.bnd, names)
        note_worst(pattern, cid, ratios)
        bad = outside(ratios)
        if bad:
            problems.append(f"slices outside the bound (err, bound): {bad}")
        # launches: nothing new, nothing more often, and exactly the table written down
        full = KEYS[cid]
        dropped = {k: full[k] - keys.get(k, 0) for k in full if keys.get(k, 0) != full[k]}
        print(f'    ("{cid}", "{pattern}"): dropped {_fmt(dropped)}, own keys {_fmt({k: n for k, n in keys.items() if k not in full})}')
        more = held_against_the_table(keys, full)
        if more:
            problems.append(f"launches the all-trainable run does not issue, key: (launched, all-trainable) {more}")
        want = expected_keys(cid, pattern)
        diff = {k: (keys.get(k, 0), want.get(k, 0)) for k in set(keys) | set(want) if keys.get(k, 0) != want.get(k, 0)}
        if diff:
            problems.append(f"launches changed, key: (launched, expected) {diff}")
        # under the flag: bit for bit the all-trainable run
        base = flagged_base(cid)
        with flagged():
            det, _ = run(data, pattern)
        have = [n for n in frozen if det.get(n) is not None]
        if have:
            problems.append(f"under the flag, frozen leaves with a gradient: {have}")
        ne = [n for n in unequal(det, base, names) if (cid, pattern, n) not in NOT_BITWISE]
        print(f"    {cid} {pattern}: not bitwise equal to the all-trainable run under the flag: {ne}")
        if ne:
            problems.append(f"not bitwise equal to the all-trainable run under the flag: {ne}")
        kept = [n for n in names if (cid, pattern, n) in NOT_BITWISE]
        if kept:
            bad = outside(ratios_against(kind, det, data.ref, data.bnd, kept))
            if bad:
                problems.append(f"under the flag, slices outside the bound: {bad}")
    assert not problems, f"{cid} {pattern}: " + "; ".join(problems)


@pytest.mark.parametrize("cid", BASE)
def test_forward_without_grad_mode(cid):
    """nothing frozen, forward under torch.no_grad() and under torch.inference_mode(): no graph, the bits of the grad-mode
    output (blocks of VENDOR_CONV: the twin's bound), no launch the grad-mode forward does not issue"""
    data = case_data(cid)
    kind = data.kind
    onames = [k for k in data.ref if k.startswith("out") and "." not in k]
    with timed(f"{cid} none-nograd"):
        base, _ = plain_base(cid)
        _reset(data)
        for mode in (torch.no_grad, torch.inference_mode):
            xs = [x.detach().clone() for x in data.xs]
            if data.seed is not None:
                torch.manual_seed(data.seed)
            with recording() as log, mode():
                outs = data.blk(*xs)
                torch.cuda.synchronize()
            outs = outs if isinstance(outs, tuple) else (outs,)
            assert not any(o.requires_grad for o in outs), f"{cid} {mode.__name__}: the output requires grad"
            got = {f"out{i}": o for i, o in enumerate(outs)}
            keys = collections.Counter(reduce_key(k) for k in log if k is not None)
            more = held_against_the_table(keys, KEYS[cid])
            assert not more, f"{cid} {mode.__name__}: launches the grad-mode run does not issue {more}"
            assert not any(k[0].endswith("bwd") for k in keys), keys
            ratios = ratios_against(kind, got, data.ref, data.bnd, onames)
            note_worst("none-nograd", cid, ratios)
            assert not outside(ratios), f"{cid} {mode.__name__}: {outside(ratios)}"
            if kind not in VENDOR_CONV:
                ne = unequal(got, base, onames)
                assert not ne, f"{cid} {mode.__name__}: not the bits of the grad-mode output: {ne}"


# ---------------------------------------------------------------------------------------------------------------------
# accumulation and repetition

def _leaves(data, xs):
    d = {f"dx{i}": x for i, x in enumerate(xs)}
    d.update(dict(data.blk.named_parameters()))
    return d


@functools.lru_cache(maxsize=None)
def retain_run(cid, flag):
    """two backwards through one retained graph, no zero_grad in between: (g1 cloned after the first call, the first
    call's .grad tensor objects, what .grad holds after the second call, outputs)"""
    data = case_data(cid)
    with (flagged() if flag else contextlib.nullcontext()):
        outs, xs = product_run(data)
        torch.autograd.backward(outs, data.gys, retain_graph=True)
        leaves = _leaves(data, xs)
        alias = {n: t.grad for n, t in leaves.items() if t.grad is not None}
        g1 = {n: g.clone() for n, g in alias.items()}
        torch.autograd.backward(outs, data.gys, retain_graph=True)
        torch.cuda.synchronize()
        g2 = {n: t.grad for n, t in leaves.items() if t.grad is not None}
        o = {f"out{i}": t.detach() for i, t in enumerate(outs)}
    _reset(data)
    return g1, alias, g2, o


def _grad_names(data):
    return [n for n in data.ref if not (n.startswith("out") and "." not in n)]


@pytest.mark.parametrize("flag", [False, True], ids=["plain", "flag"])
@pytest.mark.parametrize("cid", BASE)
def test_two_backwards_through_a_retained_graph(cid, flag):
    data = case_data(cid)
    with timed(f"{cid} retain {'flag' if flag else 'plain'}"):
        g1, alias, g2, outs = retain_run(cid, flag)
        names = _grad_names(data)
        ratios = ratios_against(data.kind, {**g2, **outs}, {**scaled(data.ref, 2.0), **{k: data.ref[k] for k in outs}}, data.bnd,
                                names + list(outs))
        note_worst("retain", cid, ratios)
        assert not outside(ratios), f"{cid}: accumulated gradients against 2 * ref: {outside(ratios)}"
        first = ratios_against(data.kind, g1, data.ref, data.bnd, names)
        assert not outside(first), f"{cid}: the first call's gradients: {outside(first)}"
        # the first call's gradient tensor either accumulated the second in place (then it IS .grad) or must still hold
        # the first call's values: a buffer the second call wrote would show here
        for n in names:
            if alias[n] is not g2[n]:
                assert torch.equal(alias[n], g1[n]), f"{cid} {n}: the first call's gradient changed under the second call"
        if flag:
            ne = [n for n in names if not torch.equal(g2[n], g1[n] + g1[n])]
            assert not ne, f"{cid}: .grad after two calls is not g1 + g1 bit for bit: {ne}"
            ne = unequal(g1, flagged_base(cid), names)
            assert not ne, f"{cid}: a retained graph changes the first call's bits: {ne}"


@functools.lru_cache(maxsize=None)
def inflight_run(cid, order, flag):
    """two forwards on two micro-batches of one block, then both backwards (order "lifo": the second graph first)"""
    da, db = case_data(cid), case_data(cid, "second")
    with (flagged() if flag else contextlib.nullcontext()):
        outs_a, xs_a = product_run(da)
        outs_b, xs_b = product_run(da, xs=db.xs)          # the same block: .grad is still empty, nothing is cleared
        steps = [(outs_a, da.gys), (outs_b, db.gys)]
        for outs, gys in (steps[::-1] if order == "lifo" else steps):
            torch.autograd.backward(outs, gys)
        torch.cuda.synchronize()
        ga = collect(da, outs_a, xs_a, missing="leave")
        gb = {k: v for k, v in collect(da, outs_b, xs_b, missing="leave").items() if k.startswith(("out", "dx")) and "." not in k}
    _reset(da)
    return ga, gb


@pytest.mark.parametrize("flag", [False, True], ids=["plain", "flag"])
@pytest.mark.parametrize("order", ["lifo", "fifo"])
@pytest.mark.parametrize("cid", BASE)
def test_two_graphs_in_flight(cid, order, flag):
    """the accumulated parameter gradients are the sum of the two micro-batches' own; each graph's outputs and input
    gradients are its own.  Both hand-off registries of sigma_amd/_handoff.py hold entries of two live graphs here."""
    da, db = case_data(cid), case_data(cid, "second")
    kind = da.kind
    with timed(f"{cid} two-in-flight {order} {'flag' if flag else 'plain'}"):
        ga, gb = inflight_run(cid, order, flag)
        own = [k for k in da.ref if k.startswith(("out", "dx")) and "." not in k]
        params = [n for n, _ in da.blk.named_parameters()]
        ra = ratios_against(kind, ga, da.ref, da.bnd, own)
        rb = ratios_against(kind, gb, db.ref, db.bnd, own)
        assert not outside(ra) and not outside(rb), f"{cid}: outputs / input gradients: {outside(ra)} {outside(rb)}"
        ref = {n: da.ref[n].double() + db.ref[n].double() for n in params}
        rs = ratios_against(kind, ga, ref, sum_bound(kind, da, db, params), params)
        note_worst("two-in-flight", cid, rs)
        assert not outside(rs), f"{cid}: accumulated gradients against refA + refB: {outside(rs)}"
        if flag:
            a, b = flagged_base(cid), flagged_base(cid, "second")
            ne = [n for n in params if not torch.equal(ga[n], a[n] + b[n])]
            assert not ne, f"{cid}: accumulated gradients are not gA + gB bit for bit: {ne}"
            assert not unequal(ga, a, own) and not unequal(gb, b, own), f"{cid}: a graph's own results changed bits"


# ---------------------------------------------------------------------------------------------------------------------
# gradient layouts

def _permuted(gy):
    """the values of gy in a tensor whose strides are those of a channels-first buffer"""
    return gy.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)


def _misaligned(gy):
    """the values of gy at a storage offset of one float: a slice of a buffer one float larger"""
    buf = torch.empty(gy.numel() + 1, device=gy.device, dtype=gy.dtype)
    v = buf[1:].view(gy.shape)
    v.copy_(gy)
    assert v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("layout", ["permuted", "misaligned"])
@pytest.mark.parametrize("cid", LAYOUT)
def test_output_gradient_layouts(cid, layout):
    data = case_data(cid)
    with timed(f"{cid} {layout}"):
        make = _permuted if layout == "permuted" else _misaligned
        gys = [make(g) for g in data.gys]
        assert all(torch.equal(a, b) for a, b in zip(gys, data.gys))
        assert all(not g.is_contiguous() for g in gys) if layout == "permuted" else True
        names = list(data.ref)
        plain, _ = run(data, gys=gys)
        ratios = ratios_against(data.kind, plain, data.ref, data.bnd, names)
        note_worst(layout, cid, ratios)
        assert not outside(ratios), f"{cid} {layout}: {outside(ratios)}"
        with flagged():
            det, _ = run(data, gys=gys)
        ne = unequal(det, flagged_base(cid), names)
        assert not ne, f"{cid} {layout}: not the bits of the contiguous delivery under the flag: {ne}"


@pytest.mark.parametrize("cid", LAYOUT)
def test_stride_zero_output_gradient(cid):
    """``out.sum().backward()``: the gradient arrives as an expanded scalar, all strides 0"""
    data = case_data(cid, "ones")
    with timed(f"{cid} stride-0"):
        outs, xs = product_run(data)
        outs[0].sum().backward()
        torch.cuda.synchronize()
        got = collect(data, outs, xs, missing="leave")
        _reset(data)
        ratios = ratios_against(data.kind, got, data.ref, data.bnd, list(data.ref))
        note_worst("stride-0", cid, ratios)
        assert not outside(ratios), f"{cid} stride-0: {outside(ratios)}"


# ---------------------------------------------------------------------------------------------------------------------
# negative controls: the checkers above on wrong references

def test_control_a_frozen_leaf_passed_off_as_trainable_fails():
    data = case_data("vss-L96")
    got, _ = run(data, "raw")
    names = trainable_names(data, "raw")
    assert not outside(ratios_against(data.kind, got, data.ref, data.bnd, names))
    with pytest.raises(AssertionError, match="no gradient for leaves"):
        ratios_against(data.kind, got, data.ref, data.bnd, names + ["op.A_logs"])


@pytest.mark.parametrize("cid", BASE)
def test_control_accumulated_gradients_fail_against_one_reference(cid):
    data = case_data(cid)
    _, _, g2, _ = retain_run(cid, False)
    names = _grad_names(data)
    ratios = ratios_against(data.kind, g2, data.ref, data.bnd, names)
    nonzero = {k for n in names for (k, s) in twin.slices(data.kind, n, data.ref[n]) if float(s.norm()) > 0}
    passed = sorted(nonzero - set(outside(ratios)))
    assert not passed, f"{cid}: 2 g passes the bound against 1 * ref on {passed}"


@pytest.mark.parametrize("cid", BASE)
def test_control_two_graphs_fail_against_twice_the_first(cid):
    da = case_data(cid)
    ga, _ = inflight_run(cid, "lifo", False)
    params = [n for n, _ in da.blk.named_parameters()]
    ref = {n: 2.0 * da.ref[n].double() for n in params}
    ratios = ratios_against(da.kind, ga, ref, sum_bound(da.kind, da, da, params), params)
    nonzero = {k for n in params for (k, s) in twin.slices(da.kind, n, da.ref[n]) if float(s.norm()) > 0}
    passed = sorted(nonzero - set(outside(ratios)))
    assert not passed, f"{cid}: gA + gB passes the bound against refA + refA on {passed}"


@pytest.mark.parametrize("cid", BASE)
def test_training_after_an_inference_mode_forward(cid):
    """the first forward of a block runs under torch.inference_mode() (nothing derived from its parameters is cached
    yet: a model that is validated before it is trained), then a training forward + backward: what the first forward
    left behind must serve the second.  The cache of parameter-derived tensors (ss2d_fused._derived_params) kept
    inference tensors here, which no later forward can save for its backward."""
    from sigma_amd import ss2d_fused
    data = case_data(cid)
    with timed(f"{cid} inference-then-train"):
        ss2d_fused.invalidate_derived_params()
        xs = [x.detach().clone() for x in data.xs]
        if data.seed is not None:
            torch.manual_seed(data.seed)
        with torch.inference_mode():
            data.blk(*xs)
        got, _ = run(data)
        ratios = ratios_against(data.kind, got, data.ref, data.bnd, list(data.ref))
        assert not outside(ratios), f"{cid}: {outside(ratios)}"
        with flagged():
            ss2d_fused.invalidate_derived_params()
            with torch.inference_mode():
                data.blk(*[x.detach().clone() for x in data.xs])
            det, _ = run(data)
        ne = unequal(det, flagged_base(cid), list(data.ref))
        assert not ne, f"{cid}: not the bits of a run without the inference-mode forward: {ne}"


# ---------------------------------------------------------------------------------------------------------------------
# Function level: one consumer / one needs_input_grad entry at a time, against fp64 torch with the bounds of
# tests/test_gemm_gpu.py (_assert_close: 3e-5 sum|a||b| per element, 2e-5 relative rms) and tests/test_stream_fp64_gpu.py
# (check: K u S).  torch materialises the gradient of an unused output of these Functions as zeros, so the ``is None``
# branches of their backwards are not reachable from here; these cases pin what actually arrives.

def _gemm_keys(log):
    return sorted(k[1] for k in log if k is not None and k[0] == "gemm")


@pytest.mark.parametrize("consumed", ["z", "x"])
@pytest.mark.parametrize("M", [96, 100])
def test_linear_xz_with_one_half_consumed(M, consumed):
    from sigma_amd import gemm
    from tests.test_gemm_gpu import _assert_close, _bound, _rand
    C, d = 64, 128
    x = _rand(M, C, seed=41).requires_grad_()
    w = _rand(2 * d, C, seed=42, scale=0.05).requires_grad_()
    b = _rand(2 * d, seed=43, scale=0.1).requires_grad_()
    assert gemm.xz_ok(x, w)
    xT, z = gemm.LinearXZFn.apply(x, w, b)
    gx, gz = _rand(d, M, seed=44), _rand(M, d, seed=45)
    x64, w64, b64 = (t.detach().double().requires_grad_() for t in (x, w, b))
    ref = torch.nn.functional.linear(x64, w64, b64)
    if consumed == "z":
        (z * gz).sum().backward()
        (ref[:, d:] * gz.double()).sum().backward()
        g2 = torch.cat([torch.zeros(M, d, device=DEV), gz], 1).double()
    else:
        (xT * gx).sum().backward()
        (ref[:, :d].t() * gx.double()).sum().backward()
        g2 = torch.cat([gx.t(), torch.zeros(M, d, device=DEV)], 1).double()
    torch.cuda.synchronize()
    _assert_close(x.grad, x64.grad, _bound(g2, w64.detach()), "dx")
    _assert_close(w.grad, w64.grad, _bound(g2.t(), x64.detach()), "dw")
    dead = slice(0, d) if consumed == "z" else slice(d, 2 * d)
    assert bool((w.grad[dead] == 0).all()) and bool((b.grad[dead] == 0).all()), "the half nobody consumed has a gradient"
    torch.testing.assert_close(b.grad.double(), b64.grad, rtol=1e-4, atol=1e-4 * float(b64.grad.abs().max()))


@pytest.mark.parametrize("needs", ["x", "weight", "bias"])
@pytest.mark.parametrize("M", [96, 100])
def test_linear_xz_with_one_input_that_needs_a_gradient(M, needs):
    """the three needs_input_grad branches of LinearXZFn.backward one at a time: the gradient of the one leaf under the
    GEMM bound, none for the others, and only that leaf's GEMMs launched in the backward"""
    from sigma_amd import gemm
    from tests.test_gemm_gpu import _assert_close, _bound, _rand
    C, d = 64, 128
    x = _rand(M, C, seed=46).requires_grad_(needs == "x")
    w = _rand(2 * d, C, seed=47, scale=0.05).requires_grad_(needs == "weight")
    b = _rand(2 * d, seed=48, scale=0.1).requires_grad_(needs == "bias")
    xT, z = gemm.LinearXZFn.apply(x, w, b)
    gx, gz = _rand(d, M, seed=49), _rand(M, d, seed=50)
    with recording() as log:
        torch.autograd.backward([xT, z], [gx, gz])
        torch.cuda.synchronize()
    g2 = torch.cat([gx.t(), gz], 1).double()
    x64, w64 = x.detach().double(), w.detach().double()
    assert [t.grad is not None for t in (x, w, b)] == [needs == "x", needs == "weight", needs == "bias"]
    if needs == "x":
        _assert_close(x.grad, g2 @ w64, _bound(g2, w64), "dx")
        assert _gemm_keys(log) == ["nn", "tn"], log
    elif needs == "weight":
        _assert_close(w.grad, g2.t() @ x64, _bound(g2.t(), x64), "dw")
        assert _gemm_keys(log) == ["nn", "tn"], log
    else:
        torch.testing.assert_close(b.grad.double(), g2.sum(0), rtol=1e-4, atol=1e-4 * float(g2.sum(0).abs().max()))
        assert _gemm_keys(log) == [], log


@pytest.mark.parametrize("consumed", ["x", "z"])
@pytest.mark.parametrize("shape", [(2, 7, 9, 128), (1, 4, 8, 64)], ids=["2x7x9x128", "1x4x8x64"])
def test_split_xz_with_one_half_consumed(shape, consumed):
    """SplitXZFn moves data only: the gradient of xz is the consumed half's gradient in its place and exact zeros in
    the other half"""
    from sigma_amd.ss2d_fused import split_xz
    from tests.test_gemm_gpu import _rand
    B, H, W, d2 = shape
    d = d2 // 2
    xz = _rand(B, H, W, d2, seed=51).requires_grad_()
    x, z = split_xz(xz)
    assert torch.equal(x, xz.detach()[..., :d].permute(0, 3, 1, 2)) and torch.equal(z, xz.detach()[..., d:])
    want = torch.zeros(B, H, W, d2, device=DEV)
    if consumed == "x":
        g = _rand(B, d, H, W, seed=52)
        x.backward(g)
        want[..., :d] = g.permute(0, 2, 3, 1)
    else:
        g = _rand(B, H, W, d, seed=53)
        z.backward(g)
        want[..., d:] = g
    torch.cuda.synchronize()
    assert torch.equal(xz.grad, want)


@pytest.mark.parametrize("consumed", ["pass", "norm"])
@pytest.mark.parametrize("shape", [(2, 8, 12, 64), (2, 7, 9, 96)], ids=["2x8x12x64", "2x7x9x96"])
def test_layernorm_residual_with_one_output_consumed(shape, consumed):
    """LayerNormResidualFn with only the handed-through input or only the normalised output consumed; bounds and their
    K, S of tests/test_stream_fp64_gpu.py::test_layernorm_against_fp64 with the gradient that does not arrive set to zero
    (so a sum whose every term is zero must be exactly zero)"""
    from sigma_amd import _capi
    from sigma_amd.layernorm import LayerNormResidualFn
    from tests.test_stream_fp64_gpu import _ln_ref, _rand, check, ln_nv
    C = shape[-1]
    rows = math.prod(shape[:-1])
    eps = 1e-5
    x = _rand(*shape, seed=61, scale=0.02, mean=0.3).requires_grad_()
    gamma = _rand(C, seed=62, scale=0.5, mean=1.0).requires_grad_()
    beta = _rand(C, seed=63, scale=0.1).requires_grad_()
    y, xp = LayerNormResidualFn.apply(x, gamma, beta, eps)
    x64, g64, b64 = (t.detach().double().reshape(-1, C).requires_grad_() if t.dim() > 1 else t.detach().double().requires_grad_()
                     for t in (x, gamma, beta))
    y64, xh, r, mu = _ln_ref(x64, g64, b64, eps)
    d = 4 * ln_nv(C) + 6
    with torch.no_grad():
        xha = xh.abs() + r * x64.abs().mean(-1, keepdim=True)
        check("layernorm", y.reshape(-1, C), y64, g64.abs() * xha + b64.abs(), d + 12, "y")
    assert torch.equal(xp, x.detach())
    if consumed == "pass":
        dadd = _rand(*shape, seed=64)
        xp.backward(dadd)
        torch.cuda.synchronize()
        dy64 = torch.zeros(rows, C, device=DEV, dtype=torch.float64)
        dadd64 = dadd.double().reshape(-1, C)
    else:
        dy = _rand(*shape, seed=65) + 25.0 * (x.detach() - x.detach().mean(-1, keepdim=True))
        y.backward(dy)
        torch.cuda.synchronize()
        dy64 = dy.double().reshape(-1, C)
        dadd64 = torch.zeros_like(dy64)
    y64.backward(dy64)
    nw = int(_capi.load().sigma_layernorm_bwd_partial_rows(rows, C))
    with torch.no_grad():
        gg = (dy64 * g64).abs()
        S_dx = r * (gg + gg.mean(-1, keepdim=True) + xha * (gg * xha).mean(-1, keepdim=True)) + dadd64.abs()
        check("layernorm", x.grad.reshape(-1, C), x64.grad + dadd64, S_dx, 2 * d + 16, "dx")
        G = max(nw, 1)
        Kc = -(-rows // (4 * G)) + -(-G // 16) + 20
        check("layernorm", gamma.grad, g64.grad, (dy64.abs() * xha).sum(0), Kc + d + 12, "dgamma")
        check("layernorm", beta.grad, b64.grad, dy64.abs().sum(0), Kc, "dbeta")
    if consumed == "pass":
        assert bool((gamma.grad == 0).all()) and bool((beta.grad == 0).all())


@pytest.mark.parametrize("fn", ["layernorm", "gated_layernorm", "scale_residual", "linear"])
def test_packed_gradient_off_a_16_byte_boundary(fn):
    """a packed output gradient one float into a larger buffer, handed straight to the Functions whose kernels load 16
    bytes per lane: the bits of the aligned delivery under the flag (the values are the fp64 tests' business).
    ScaleResidualFn raised here (the kernel refuses the pointer) and LinearSplit3Fn sent its GEMMs to the vendor library."""
    from sigma_amd import gemm
    from sigma_amd.layernorm import LayerNorm
    from sigma_amd.pointwise import scale_residual
    from tests.test_gemm_gpu import _rand
    shape, C = (2, 7, 9, 96), 96
    x0, a0, z0 = _rand(*shape, seed=81), _rand(*shape, seed=82), _rand(*shape, seed=86)
    gy = _rand(*shape, seed=83)
    ln = LayerNorm(C).to(DEV)
    w0, s0 = _rand(192, C, seed=84, scale=0.05), _rand(C, seed=85)

    def once(g):
        leaves = [t.clone().requires_grad_() for t in (x0, a0, z0, w0, s0)]
        x, a, z, w, sc = leaves
        for p in ln.parameters():
            p.grad = None
        if fn == "layernorm":
            y = ln(x)
        elif fn == "gated_layernorm":
            y = ln.forward_gated(x, z)
        elif fn == "scale_residual":
            y = scale_residual(a, x, sc)
        else:
            y = gemm.linear(x, w)
        with recording() as log:
            y.backward(g)
            torch.cuda.synchronize()
        return [t.grad for t in leaves + list(ln.parameters()) if t.grad is not None], [k[:2] for k in log if k is not None]

    with flagged():
        if fn == "linear":
            g2 = torch.cat([gy, gy], -1)
            want, keys = once(g2)
            got, keys_m = once(_misaligned(g2))
        else:
            want, keys = once(gy)
            got, keys_m = once(_misaligned(gy))
    assert len(want) == len(got) and len(want) >= 2
    assert all(torch.equal(a, b) for a, b in zip(want, got)), "a gradient off the 16-byte boundary changes the bits"
    assert keys and keys == keys_m, (keys, keys_m)


@pytest.mark.parametrize("needs", ["x", "weight", "bias", "residual"])
def test_linear_split3_with_one_input_that_needs_a_gradient(needs):
    """the four needs_input_grad branches of LinearSplit3Fn.backward one at a time (C = 96, odd row count)"""
    from sigma_amd import gemm
    from tests.test_gemm_gpu import _assert_close, _bound, _rand
    M, K, N = 2 * 9 * 11, 96, 192
    x = _rand(M, K, seed=71).requires_grad_(needs == "x")
    w = _rand(N, K, seed=72, scale=0.05).requires_grad_(needs == "weight")
    b = _rand(N, seed=73, scale=0.1).requires_grad_(needs == "bias")
    res = _rand(M, N, seed=74).requires_grad_(needs == "residual")
    gy = _rand(M, N, seed=75)
    y = gemm.LinearSplit3Fn.apply(x, w, b, res)
    x64, w64, g64 = x.detach().double(), w.detach().double(), gy.double()
    y64 = x64 @ w64.t() + b.detach().double() + res.detach().double()
    _assert_close(y.detach(), y64, _bound(x64, w64.t()) + b.detach().double().abs() + res.detach().double().abs(), "y")
    with recording() as log:
        y.backward(gy)
        torch.cuda.synchronize()
    leaves = dict(x=x, weight=w, bias=b, residual=res)
    assert {n for n, t in leaves.items() if t.grad is not None} == {needs}
    if needs == "x":
        _assert_close(x.grad, g64 @ w64, _bound(g64, w64), "dx")
    elif needs == "weight":
        _assert_close(w.grad, g64.t() @ x64, _bound(g64.t(), x64), "dw")
    elif needs == "bias":
        torch.testing.assert_close(b.grad.double(), g64.sum(0), rtol=1e-4, atol=1e-4 * float(g64.sum(0).abs().max()))
    else:
        assert torch.equal(res.grad, gy)
    assert _gemm_keys(log) == {"x": ["nn"], "weight": ["tn"], "bias": [], "residual": []}[needs], log


@pytest.mark.parametrize("needs", ["x", "weight"])
@pytest.mark.parametrize("route", ["loss", "elsewhere"])
@pytest.mark.parametrize("nc", [5, 9])
def test_classifier_with_one_input_that_needs_a_gradient(nc, route, needs):
    """the two needs_input_grad branches of ClassifierPadFn.backward one at a time, with the gradient handed over by the
    loss (padded buffer, _handoff.py) and with one from elsewhere (copying path); the classes 5 and 9 at C = 96"""
    import torch.nn.functional as F
    from sigma_amd import gemm
    from sigma_amd.pointwise import cross_entropy
    from tests.test_gemm_gpu import _assert_close, _bound
    from tests.test_head_classes_gpu import IGNORE, _head_inputs
    C = 96
    x0, w0, label = _head_inputs(nc, C, seed=231)
    B, H, W = x0.shape[:3]
    x = x0.clone().requires_grad_(needs == "x")
    w = torch.nn.Parameter(w0.clone(), requires_grad=needs == "weight")
    x64, w64 = x0.double().reshape(-1, C), w0.double().view(nc, C)
    logits = gemm.classifier(x, w)
    if route == "loss":
        z64 = (x64 @ w64.t()).requires_grad_()
        F.cross_entropy(z64, label.view(-1), ignore_index=IGNORE).backward()
        g64 = z64.grad
        loss = cross_entropy(torch.nn.CrossEntropyLoss(reduction="mean", ignore_index=IGNORE), logits.permute(0, 3, 1, 2), label)
        assert loss is not None
        with recording() as log:
            loss.backward()
    else:
        g = torch.randn(B, nc, H, W, generator=torch.Generator().manual_seed(232)).to(DEV)
        g64 = g.double().permute(0, 2, 3, 1).reshape(-1, nc)
        with recording() as log:
            logits.permute(0, 3, 1, 2).backward(g)
    torch.cuda.synchronize()
    assert (x.grad is not None, w.grad is not None) == (needs == "x", needs == "weight")
    if needs == "x":
        _assert_close(x.grad.reshape(-1, C), g64 @ w64, _bound(g64, w64), "x.grad")
        assert _gemm_keys(log) == ["nn"], log
    else:
        _assert_close(w.grad.view(nc, C), g64.t() @ x64, _bound(g64.t(), x64), "weight.grad")
        assert w.grad.is_contiguous() and tuple(w.grad.shape) == (nc, C, 1, 1)
        assert _gemm_keys(log) == ["tn"], log


def _families():
    from tests.test_deterministic_gpu import FAMILIES
    return FAMILIES


@pytest.mark.parametrize("shape", _families(), ids=[f"{s[9]}-{s[0]}x{s[1]}x{s[2]}xN{s[3]}-{str(s[8])[6:]}-p{s[7]}" for s in _families()])
def test_forward_without_checkpoints_returns_the_same_bits(shape):
    """fwd_ext(need_x=False) -- what every no-grad forward runs: a NULL checkpoint pointer -- for every forward family:
    the bits of the forward that writes checkpoints, an empty x, the same census key"""
    from sigma_amd import selective_scan_cuda_core as core
    from tests.test_deterministic_gpu import _problem
    batch, KD, L, N, G, mask, ush, pitch, dtype, _ = shape
    u, delta, A, B, C, D, bias, _ = _problem(batch, KD, L, N, G, ush, dtype, seed=3)
    args = (u, delta, A, B, C, D, bias)
    with recording() as with_x:
        out, x = core.fwd_ext(*args, True, rev_mask=mask, u_gshift=ush, ckpt_pitch=pitch)
    with recording() as without:
        out0, x0 = core.fwd_ext(*args, True, rev_mask=mask, u_gshift=ush, ckpt_pitch=pitch, need_x=False)
    torch.cuda.synchronize()
    assert x.numel() > 0 and x0.numel() == 0
    assert torch.isfinite(out0.float()).all()
    assert torch.equal(out, out0), "the forward without checkpoints returns other bits"
    assert len(with_x) == 1 and with_x == without, (with_x, without)


# ---------------------------------------------------------------------------------------------------------------------
# model level

def test_model_autograd_contract():
    """tests/autograd_contract_worker.py: the fixture model under freeze patterns, accumulation and two micro-batches in
    flight, under torch's flag, in one child process (the flag and CUBLAS_WORKSPACE_CONFIG stay out of this one)"""
    env = dict(os.environ, CUBLAS_WORKSPACE_CONFIG=":4096:8", SIGMA_GEMM="split3")
    env.pop("SIGMA_CKPT_PITCH", None)
    r = subprocess.run([sys.executable, "-m", "tests.autograd_contract_worker"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"worker exit {r.returncode}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    assert "[autograd_contract_worker] done" in r.stdout


def test_zz_report_worst_ratios_and_seconds():
    """prints the worst err / bound of each pattern (asserted <= 1 above) and the seconds of every case; DESIGN.md 4.7b
    quotes them"""
    print("\nworst err / bound per pattern:")
    for pattern, (r, where) in sorted(WORST.items()):
        print(f"   {pattern:14s} {r:.3g}   {where}")
    print(f"seconds: {sum(SECONDS.values()):.1f} in {len(SECONDS)} timed cases; slowest:")
    for what, s in sorted(SECONDS.items(), key=lambda kv: -kv[1])[:8]:
        print(f"   {s:6.2f}  {what}")
