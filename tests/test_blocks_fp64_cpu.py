"""The fp64 block twins (tests/block_fp64_twin.py) on the CPU: anchored to the original project's own blocks, and able
to see the defects they are there to catch.  Only reference code runs here.

* the twin's selective scan passes ``torch.autograd.gradcheck`` in fp64;
* the twin reproduces every fixture of tests/golden/make_golden_blocks.py (the original's blocks, run unmodified on CPU)
  within 16 * max(e32, 2^-23) per slice, e32 = the float32 twin against the float64 twin on the same data: both sides
  are fp32-class computations of one function in different operation orders;
* every wrong variant of WRONG differs from the right twin by more than the bound a kernel-built block is allowed,
  2 (e32 + e_pert) + 2^-23, in the slice it names;
* the noise mode is reproducible by seed.
"""
from __future__ import annotations

import ast
import functools
import os

import numpy as np
import pytest
import torch

from tests import block_fp64_twin as twin
from tests.model_utils import GOLDEN, fill

FIXTURES = ["vss_eval", "vss_train", "cromb_eval", "cromb_train", "conmb_eval", "conmb_train", "cvss_eval", "merge_odd"]


@functools.lru_cache(maxsize=None)
def _fixture(name):
    z = np.load(os.path.join(GOLDEN, f"block_{name}.npz"), allow_pickle=False)
    meta = ast.literal_eval(str(z["meta"]))
    t = lambda k: torch.from_numpy(z[k])
    names = [str(n) for n in z["param_names"]]
    sd = {n: fill.value_for(n, z["g:" + n].shape) for n in names}
    n_in = sum(1 for k in z.files if k.startswith("x") and k[1:].isdigit())
    n_out = sum(1 for k in z.files if k.startswith("gy"))
    xs, gys = [t(f"x{i}") for i in range(n_in)], [t(f"gy{i}") for i in range(n_out)]
    factors = [f for f in t("factors")] if z["factors"].shape[0] else None
    want = {f"out{i}": t(f"out{i}") for i in range(n_out)}
    want.update({f"dx{i}": t(f"dx{i}") for i in range(n_in)})
    want.update({n: t("g:" + n) for n in names})
    return meta["kind"], sd, xs, gys, factors, want


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(ref64, e32, e_pert) of a fixture's data, computed once and shared (never modified)"""
    kind, sd, xs, gys, factors, _ = _fixture(name)
    return twin.twin_reference(kind, sd, xs, gys, factors)


def test_twin_scan_passes_gradcheck():
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Bsz, G, rows, N, L = 2, 2, 3, 2, 7
    u, delta = r(Bsz, G * rows, L).requires_grad_(), (0.5 * r(Bsz, G * rows, L)).requires_grad_()
    A = (-torch.rand(G * rows, N, generator=g, dtype=torch.float64) - 0.2).requires_grad_()
    Bm, Cm = r(Bsz, G, N, L).requires_grad_(), r(Bsz, G, N, L).requires_grad_()
    D, bias = r(G * rows).requires_grad_(), (r(G * rows) - 1.0).requires_grad_()
    assert torch.autograd.gradcheck(twin.selective_scan, (u, delta, A, Bm, Cm, D, bias), eps=1e-6, atol=1e-7, rtol=1e-5)
    # and the recurrence is the recurrence: against the loop over the sequence
    a, w = torch.rand(3, 11, generator=g, dtype=torch.float64), r(3, 11)
    h, want = torch.zeros(3, dtype=torch.float64), []
    for t in range(11):
        h = a[:, t] * h + w[:, t]
        want.append(h)
    torch.testing.assert_close(twin.recurrence(a, w), torch.stack(want, -1), rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("name", FIXTURES)
def test_twin_reproduces_the_original_projects_block(name):
    kind, sd, xs, gys, factors, want = _fixture(name)
    ref, e32, _ = _reference(name)
    assert sorted(ref) == sorted(want)
    err = twin.slice_errors(kind, want, ref)
    bad = {}
    print()
    for k in sorted(err):
        b = 16.0 * max(e32[k], twin.U23)
        print(f"  {name} {k:44s} err {err[k]:.3g}  bound {b:.3g}")
        if not err[k] <= b:
            bad[k] = (err[k], b)
    assert not bad, f"twin and original differ: {bad}"


# defect -> the slices under its named tensor that must leave the bound: all of them where the defect touches every
# sample / direction; in the training-mode VSS fixture sample 0 is dropped and sample 1 kept, so a defect inside the
# branch shows in sample 1 alone, while the missing residual gradient shows in both
FAILS = {
    "dt_weight_perm": ["[k=1]", "[k=2]"],              # the two exchanged directions; 0 and 3 stay exact
    "dA_no_A": ["[k=0]", "[k=1]", "[k=2]", "[k=3]"],
    "du_rev_dropped": ["[b=1]"],
    "residual_grad": ["[b=0]", "[b=1]"],
    "mask_unscaled": ["[b=1]"],                        # the dropped sample is untouched, the kept one is wrong
    "pair_one_direction": ["[k=1]"],                   # the reversed direction gets nothing; the forward one stays exact
    "c_not_swapped": ["[b=0]", "[b=1]"],
    "scale1_operand": [""],
    "merge_order": ["[b=0]", "[b=1]"],
}


@pytest.mark.parametrize("wrong", sorted(twin.WRONG))
def test_wrong_variant_leaves_the_bound_in_its_slice(wrong):
    kind, where = twin.WRONG[wrong]
    name = {"vss": "vss_train", "cvss": "cvss_eval", "cromb": "cromb_eval", "conmb": "conmb_eval", "merge": "merge_odd"}[kind]
    _, sd, xs, gys, factors, _ = _fixture(name)
    if name == "vss_train":
        assert [float(f) != 0.0 for f in factors[0]] == [False, True]
    ref, e32, e_pert = _reference(name)
    bnd = twin.bound(e32, e_pert)
    err = twin.slice_errors(kind, twin.run(kind, sd, xs, gys, factors, wrong=wrong), ref)
    under = {k: (err[k], bnd[k]) for k in err if k == where or k.startswith(where + "[")}
    hit = sorted(k for k, (e, b) in under.items() if e > b)
    assert hit == sorted(where + s for s in FAILS[wrong]), f"{wrong}: slices of {where} outside the bound: {hit}; all: {under}"
    if wrong in ("dt_weight_perm", "pair_one_direction"):
        assert all(e == 0.0 for k, (e, _) in under.items() if k not in hit), under
    # the bound is orders of magnitude below a structural error
    assert max(bnd.values()) < 1e-2, max(bnd.values())


def test_noise_mode_is_reproducible_by_seed():
    kind, sd, xs, gys, factors, _ = _fixture("vss_eval")
    a = twin.run(kind, sd, xs, gys, factors, noise_seed=7)
    b = twin.run(kind, sd, xs, gys, factors, noise_seed=7)
    c = twin.run(kind, sd, xs, gys, factors, noise_seed=8)
    clean = _reference("vss_eval")[0]
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], c[k]) for k in a)
    e = twin.slice_errors(kind, a, clean)
    assert all(0.0 < v < 1e-2 for v in e.values()), e          # every slice is downstream of some product; sigma = 2e-5
    again = twin.run(kind, sd, xs, gys, factors)                # and the switch leaves nothing behind
    assert all(torch.equal(again[k], clean[k]) for k in clean)
