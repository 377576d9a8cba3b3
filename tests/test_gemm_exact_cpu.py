"""CPU half of the exact GEMM suite (tests/gemm_exact_ref.py, tests/test_gemm_exact_gpu.py): the builder's properties,
sensitivity controls on reference code only, and the coverage table -- the GPU file's case list planned with
sigma_gemm_plan (host only) must reach all 24 kernel instantiations in every regime their form admits."""
import collections
import ctypes

import pytest
import torch

from sigma_amd import _capi
from tests import gemm_exact_ref as ref
from tests.gemm_exact_ref import exact_operand, exact_product, kept_products, pieces_of, unit_of
from tests.test_gemm_exact_gpu import CASES, INSTANTIATIONS


# ---------------------------------------------------------------------------------------------------------------------
# builder properties

@pytest.mark.parametrize("kind,P", [("unit", 2), ("wide", 2), ("three", 3)])
def test_pieces_reproduce_the_operand_and_are_non_trivial(kind, P):
    x = exact_operand((67, 52), P, seed=5, kind=kind)
    ps = pieces_of(x, P)
    assert torch.equal(sum(p.double() for p in ps), x.double())
    assert all(bool((p != 0).any()) for p in ps)
    assert bool((ps[0].abs() >= 1024).all()) and float(ps[-1].abs().max()) <= 3          # hi carries the scale, lo is small
    if kind == "unit":
        assert set(ps[0].abs().unique().tolist()) == {1024.0} and set(ps[1].unique().tolist()) == {-1.0, 0.0, 1.0}
    if kind == "three":
        assert set(ps[0].abs().unique().tolist()) == {2.0 ** 18} and set(ps[1].abs().unique().tolist()) == {512.0, 768.0}
    half = exact_operand((400, 50), P, seed=6, density=0.5, kind=kind)
    assert 0.4 < float((half != 0).float().mean()) < 0.6


def test_binade_trap():
    """hi + lo must stay in the binade of hi: 2^18 - 2^9 - 1 rounds to 255 * 2^10, not to 2^18"""
    x = torch.tensor([2.0 ** 18 - 2 ** 9 - 1])
    assert float(pieces_of(x, 2)[0]) == 255 * 2 ** 10


def test_units_are_derived_from_the_pieces():
    for kind, P, unit in (("unit", 2, 2 ** 10), ("wide", 2, 2 ** 10), ("three", 3, 2 ** 16)):
        a, b = exact_operand((1, 40, 36), P, 1, kind=kind), exact_operand((1, 44, 36), P, 2, kind=kind)
        assert unit_of(pieces_of(a, P), pieces_of(b, P)) == unit, kind


def test_window_assertion_fires_on_a_reduction_that_is_too_long():
    a, b = exact_operand((1, 8, 4000), 2, 1), exact_operand((1, 8, 4000), 2, 2)
    with pytest.raises(AssertionError, match="outside the 2\\^24 window"):
        exact_product("nt", a, b, 2)
    a, b = exact_operand((1, 8, 32), 3, 1), exact_operand((1, 8, 32), 3, 2)
    with pytest.raises(AssertionError, match="outside the 2\\^24 window"):
        exact_product("nt", a, b, 3)
    exact_product("nt", a[:, :, :12].contiguous(), b[:, :, :12].contiguous(), 3)          # the short dense one fits
    off_grid = torch.ones(1, 8, 8)
    with pytest.raises(AssertionError, match="off the unit grid"):
        exact_product("nt", a[:, :, :12].contiguous(), b[:, :, :12].contiguous(), 3, residuals=(off_grid,))


def _int_reference(form, A, B, P, a_mod=0):
    """the kept-pair sum in int64, pair by pair"""
    Z = B.shape[0]
    if a_mod:
        A = A[torch.arange(Z) % a_mod]
    pa, pb = [p.to(torch.int64) for p in pieces_of(A, P)], [p.to(torch.int64) for p in pieces_of(B, P)]
    out = 0
    for qa in range(P):
        for qb in range(P - qa):
            out = out + ref._mm(form, pa[qa], pb[qb])
    return out


@pytest.mark.parametrize("form,P", [(f, P) for f in ("nt", "nn", "tn") for P in (2, 3)])
def test_fp64_reference_equals_int64_arithmetic(form, P):
    M, N, K = (12, 24, 20) if form == "tn" else (24, 20, 12)                        # a reduction of 12: dense three-piece operands fit
    c = ref.Case(name="t", form=form, M=M, N=N, K=K, pieces=P, batch=4, a_mod=2 if form != "tn" else 0, seed=3)
    o = c.operands()
    want, _, _ = exact_product(form, o["A"], o["B"], P, a_mod=c.a_mod)
    got = _int_reference(form, o["A"], o["B"], P, c.a_mod)
    assert torch.equal(want.to(torch.int64), got) and torch.equal(want, got.double())


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity controls: plausible wrong variants, on reference code only; each must differ from the reference in at
# least one element of the case meant to catch it (the GPU test asserts equality, so any difference is a failure there)

def _nt_case(M=130, N=130, K=68, P=2, seed=7):
    a, b = exact_operand((1, M, K + 4), P, seed), exact_operand((1, N, K + 4), P, seed + 1)
    return a, b, a[:, :, :K].contiguous(), b[:, :, :K].contiguous()


def _pieces64(x, P=2):
    return [p.double() for p in pieces_of(x, P)]


def test_control_lo_hi_dropped_in_one_k_block():
    _, _, a, b = _nt_case()
    want = exact_product("nt", a, b, 2)[0]
    (ah, al), (bh, bl) = _pieces64(a), _pieces64(b)
    wrong = want.clone()
    wrong[:, 128:, :] -= ref._mm("nt", al[:, 128:, 16:32], bh[:, :, 16:32])           # last row tile, second k-block of step 0
    assert not torch.equal(wrong, want)
    wrong = want.clone()
    wrong[:, :, :] -= ref._mm("nt", al[:, :, 64:68], bh[:, :, 64:68])                 # the partial k-step only
    assert not torch.equal(wrong, want)


def test_control_lo_lo_added():
    for P in (2, 3):
        _, _, a, b = _nt_case(M=40, N=36, K=12, P=P)
        want = exact_product("nt", a, b, P)[0]
        dropped = [(qa, P - qa) for qa in range(1, P)]                                 # the largest dropped pairs: lo*lo; mid*lo, lo*mid
        wrong = want + kept_products("nt", a, b, P, pairs=dropped)[0]
        assert not torch.equal(wrong, want)


def test_control_lo_image_of_the_wrong_operand():
    _, _, a, b = _nt_case()                                                            # M == N: the images have the same shape
    want = exact_product("nt", a, b, 2)[0]
    (ah, al), (bh, bl) = _pieces64(a), _pieces64(b)
    wrong = ref._mm("nt", ah, bh) + ref._mm("nt", ah, al) + ref._mm("nt", bl, bh)      # lo images of A and B swapped
    assert not torch.equal(wrong, want)


def test_control_truncating_split():
    _, _, a, b = _nt_case()
    want = exact_product("nt", a, b, 2)[0]

    def trunc_pieces(x):
        hi = (x.view(torch.int32) & -65536).view(torch.float32)
        r = x - hi
        return hi.double(), (r.view(torch.int32) & -65536).view(torch.float32).double()
    (ah, al), (bh, bl) = trunc_pieces(a), trunc_pieces(b)
    wrong = ref._mm("nt", ah, bh) + ref._mm("nt", ah, bl) + ref._mm("nt", al, bh)
    assert not torch.equal(wrong, want)


def test_control_reduction_one_element_too_long_or_too_short():
    af, bf, a, b = _nt_case()
    K = a.shape[2]
    want = exact_product("nt", a, b, 2)[0]
    assert not torch.equal(exact_product("nt", af[:, :, :K + 1].contiguous(), bf[:, :, :K + 1].contiguous(), 2)[0], want)
    assert not torch.equal(exact_product("nt", a[:, :, :K - 1].contiguous(), b[:, :, :K - 1].contiguous(), 2)[0], want)
    # every single output element moves (a nonzero kept product is never lost among the others): dense operands
    assert bool((exact_product("nt", a[:, :, :K - 1].contiguous(), b[:, :, :K - 1].contiguous(), 2)[0] != want).all())


def test_control_rows_of_a_ragged_tile_swapped():
    _, _, a, b = _nt_case()
    want = exact_product("nt", a, b, 2)[0]
    wrong = want.clone()
    wrong[:, [128, 129]] = want[:, [129, 128]]
    assert not torch.equal(wrong, want)


def test_control_bias_once_per_slice():
    c = next(c for c in CASES if c.name == "nn2-64-fx-rows-store-bias-res0")
    o = c.operands()
    want = c.reference(o)[0]
    assert not torch.equal(want + o["bias"].double(), want)                            # a second slice adding the bias again
    assert int((o["bias"] != 0).sum()) >= o["bias"].numel() - 2                        # ... moves (almost) every column


def test_control_ragged_c_mod_group_in_the_wrong_output():
    c = next(c for c in CASES if c.name == "nt2-64-e-c_mod-ragged")
    o = c.operands()
    want = c.reference(o)[0]
    per_problem = kept_products("nt", o["A"], o["B"], 2)[0]
    wrong = torch.zeros_like(want)
    for z in range(c.batch):
        wrong[(z % c.c_mod) if z < c.batch - 1 else 1] += per_problem[z]              # problem 4 belongs to output 0
    assert not torch.equal(wrong, want)


# ---------------------------------------------------------------------------------------------------------------------
# every small case stays inside the window (the large ones are asserted on the device before their launch)

_SMALL = [c for c in CASES if c.batch * c.M * c.N * c.K < 2e7]


@pytest.mark.parametrize("case", _SMALL, ids=[c.name for c in _SMALL])
def test_small_cases_are_inside_the_window(case):
    o = case.operands()
    _, fill = case.reference(o)                       # asserts pieces, unit grid and window
    assert 0 < fill < 1


# ---------------------------------------------------------------------------------------------------------------------
# coverage table

def xcd_logical_block(hw, nblk):
    """csrc/scan_device.h xcd_logical_block"""
    q, rem = nblk >> 3, nblk & 7
    xcd, slot = hw & 7, hw >> 3
    return (xcd * (q + 1) if xcd < rem else rem * (q + 1) + (xcd - rem) * q) + slot


def _alternates(case, plan):
    """items > 1024 and, for every grid the launch code can pick (256 x 1..4 resident workgroups per CU), the item streams
    of the workgroups (gemm_split3_kernel decode) step from a full tile to a ragged one and from a ragged one to a full one"""
    mr, nc, _ = case.kernel_dims
    ntm, ntn, sl, bn, items = plan["ntm"], plan["ntn"], plan["slices"], plan["bn"], plan["items"]
    if items <= 1024 or sl != 1:
        return False
    per_z = ntm * ntn

    def ragged(item):
        r0 = xcd_logical_block(item, items) % per_z
        tm, tn = r0 // ntn, r0 % ntn
        return (tm == ntm - 1 and mr % 128 != 0) or (tn == ntn - 1 and nc % bn != 0)
    for grid in (256, 512, 768, 1024):
        into = out_of = False
        for wg in range(grid):
            kinds = [ragged(i) for i in range(wg, items, grid)]
            into |= any(y and not x for x, y in zip(kinds, kinds[1:]))
            out_of |= any(x and not y for x, y in zip(kinds, kinds[1:]))
        if not (into and out_of):
            return False
    return True


def regimes(case, plan):
    """the regimes of the issue's list a case exercises, from its geometry and the planner's report"""
    mr, nc, kr = case.kernel_dims
    bn, sl = plan["bn"], plan["slices"]
    t = set()
    if mr % 128 == 0 and nc % bn == 0 and kr % 32 == 0 and plan["items"] == 1:
        t.add("a-full")
    if mr % 128:
        t.add("b-ragged-rows")
    if nc % bn:
        t.add("b-ragged-columns")
    if sl == 1:
        if kr < 32:
            t.add("b-k<32")
        elif kr % 32 in (4, 28):
            t.add(f"b-k=32j+{kr % 32}")
    if case.form == "nt" and mr < 32:
        t.add("b-m<32")
    if case.form == "nt" and mr == 1:
        t.add("b-m=1")
    if _alternates(case, plan):
        t.add("c-persistent")
    if sl > 1 and kr % plan["slice_k"]:
        t.add("d-two-stage" if plan["two_stage"] else "d-short-scratch" if case.ws == "short" else
              "d-atomic-accumulate" if case.accumulate else "d-atomic-zero")
    if case.batch > 1:
        t.add("e-batch")
        if 0 < case.a_mod < case.batch and case.form != "tn":
            t.add("e-a_mod")
        if case.c_mod >= case.batch:
            t.add("e-c_mod>=batch")
        elif case.c_mod > 0:
            t.add("e-c_mod-exact" if case.batch % case.c_mod == 0 else "e-c_mod-ragged")
    t.add("f-epilogue-" + plan["epilogue"])
    t.add("f-store-" + plan["store"])
    t.add("f-bias" if case.bias else "f-no-bias")
    if plan["res"]:
        t.add(f"f-res{case.res}-{plan['res_load']}")
    if case.t_cols:
        t.add("f-t_cols=N" if case.t_cols == nc else "f-t_cols<N")
        if case.t_cols % bn:
            t.add("f-t_cols-straddles-a-tile")
    if plan["epilogue"] == "direct" and plan["store"] != "atomic":
        L = case.layout()
        for why, hit in (("N%4", nc % 4 != 0), ("ldc%4", L["ldc"] % 4 != 0), ("strideC%4", case.batch > 1 and L["sC"] % 4 != 0),
                         ("misaligned-C", case.c_off % 4 != 0)):
            if hit:
                t.add("f-direct-by-" + why)
    return t


def required(inst):
    form, P, bn, res = inst
    need = {"a-full", "b-ragged-rows", "b-ragged-columns", "b-k<32", "b-k=32j+4", "b-k=32j+28", "c-persistent", "e-batch",
            "f-epilogue-rows", "f-epilogue-direct", "f-store-store", "f-store-accumulate", "f-no-bias",
            "f-direct-by-ldc%4", "f-direct-by-strideC%4", "f-direct-by-misaligned-C"}
    if form == "nt":
        need |= {"b-m<32", "b-m=1", "f-direct-by-N%4"}
    if form != "tn":
        need |= {"e-a_mod", "e-c_mod>=batch", "f-bias"}
        if not res:
            need |= {"e-c_mod-exact", "e-c_mod-ragged"}
    if not res:
        need |= {"f-store-atomic"}
    if form != "nt" and not res:
        need |= {"d-two-stage", "d-atomic-zero", "d-atomic-accumulate", "d-short-scratch"}
    if res:
        need |= {f"f-res{n}-{how}" for n in (1, 2) for how in ("vector", "scalar")}
    if form == "nt" and not res:
        need |= {"f-t_cols=N", "f-t_cols<N", "f-t_cols-straddles-a-tile"}
    return need


def coverage(cases):
    """(instantiation -> regimes reached, list of complaints) of a case list"""
    lib = _capi.load()
    table, wrong = collections.defaultdict(set), []
    combos = set()
    for c in cases:
        plan = c.plan(lib)
        if plan is None:
            wrong.append(f"{c.name}: refused by the planner")
            continue
        inst = (c.form, plan["pieces"], plan["bn"], plan["res"])
        # the relation the `stage` labels rest on: the size query asks for scratch exactly for the summed launches, and a
        # summed launch is two-stage exactly when it is given all of that scratch
        need = int(lib.sigma_gemm_workspace_bytes(ctypes.byref(c.params(c.FAKE)), _capi.GEMM_FORMS[c.form]))
        if (need > 0) != plan["summed"]:
            wrong.append(f"{c.name}: the size query answers {need} for a launch planned with summed={plan['summed']}")
        if plan["two_stage"] != (plan["summed"] and c.ws == "query"):
            wrong.append(f"{c.name}: two_stage={plan['two_stage']} with summed={plan['summed']} and the scratch {c.ws!r}")
        if (plan["bn"], plan["res"]) != tuple(c.variant) or plan["pieces"] != c.pieces:
            wrong.append(f"{c.name}: plans to {inst}, not to the variant it names {c.variant}")
        table[inst] |= regimes(c, plan)
        combos.add((c.form, plan["epilogue"], plan["store"], c.bias, c.res, plan["res_load"]))
    for inst in INSTANTIATIONS:
        if inst not in table:
            wrong.append(f"instantiation {inst} is never launched")
        elif required(inst) - table[inst]:
            wrong.append(f"instantiation {inst} misses the regimes {sorted(required(inst) - table[inst])}")
    # every epilogue kind x store mode the planner can produce, and on the linear forms every combination with bias and
    # residuals that plan_nt / plan_nn admit (summed launches take neither; the residual kernels are two-piece)
    for form in ("nt", "nn", "tn"):
        for ep, st in (("rows", "store"), ("rows", "accumulate"), ("direct", "store"), ("direct", "accumulate"), ("direct", "atomic")):
            if not any(k[:3] == (form, ep, st) for k in combos):
                wrong.append(f"{form}: epilogue {ep} x {st} never occurs")
    for bias in (False, True):
        if ("nt", "transposed", "store", bias, 0, "none") not in combos:
            wrong.append(f"nt: transposed epilogue with bias={bias} never occurs")
    for form in ("nt", "nn"):
        for ep in ("rows", "direct"):
            for st in ("store", "accumulate"):
                for bias in (False, True):
                    for nres, load in ((0, "none"), (1, "vector"), (2, "vector"), (1, "scalar"), (2, "scalar")):
                        if (form, ep, st, bias, nres, load) not in combos:
                            wrong.append(f"{form}: epilogue {ep} x {st} x bias={bias} x residuals={nres} ({load} loads) never occurs")
    return table, wrong


def test_case_list_reaches_every_instantiation_in_every_regime():
    assert len(INSTANTIATIONS) == 24 and len(set(INSTANTIATIONS)) == 24
    table, wrong = coverage(CASES)
    assert not wrong, "\n".join(wrong)
    assert set(table) == set(INSTANTIATIONS)


@pytest.mark.parametrize("name,complaint", [
    ("tn3-64-a-full", "'a-full'"), ("nn2-96r-f-res1-scalar-strideR", None), ("nt3-96-c-persistent", "'c-persistent'"),
    ("tn2-96-d-short-scratch", "'d-short-scratch'"), ("nn2-64r-fx-direct-acc-bias-res2s", "residuals=2 (scalar loads)")])
def test_deleting_a_case_names_what_became_uncovered(name, complaint):
    """the table is tight where it is meant to be: without a case that alone carries a regime, the complaint names it"""
    assert any(c.name == name for c in CASES)
    _, wrong = coverage([c for c in CASES if c.name != name])
    if complaint is None:
        assert not wrong                      # this regime has a second case
    else:
        assert any(complaint in w and name.split("-")[0][:2] in w for w in wrong), wrong


def test_real_shapes_are_in_the_list_once_each():
    g = [c for c in CASES if "-g-" in c.name]
    shapes = {(c.form, c.M, c.N, c.K, c.batch, c.bias, c.t_cols) for c in g}
    for want in (("nt", 19200, 1536, 384, 1, False, 0), ("nt", 19200, 1536, 384, 1, True, 0), ("nt", 19200, 1536, 384, 1, True, 768),
                 ("nn", 19200, 384, 1536, 1, False, 0), ("tn", 19200, 1536, 384, 1, False, 0), ("tn", 76800, 384, 96, 1, False, 0),
                 ("nn", 112, 1200, 768, 4, False, 0), ("nn", 768, 1200, 24, 8, False, 0)):
        assert want in shapes, want
    assert len(g) == len(shapes)


# ------------------------------------------------------------------------------------ the edges of the split (header formula)
def _bits(pattern):
    return torch.tensor([pattern], dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize("P", [2, 3])
def test_pieces_of_a_non_finite_or_overflowing_element(P):
    """include/sigma_gemm.h, contract difference from an fp32 GEMM: by the header's formula an element of +-inf has the
    pieces (+-inf, NaN, NaN), and a FINITE element at or above bit pattern 0x7F7F8000 (about 3.396e38), which rounds to inf
    in bf16, has (+-inf, -+inf, NaN): either way hi * b + lo * b is NaN for every b, where an fp32 GEMM returns +-inf or
    a finite value.  0x7F7F7FFF, the largest safe pattern, splits into finite pieces that add up to it."""
    inf = float("inf")
    for s in (1.0, -1.0):
        ps = pieces_of(torch.tensor([s * inf]), P)
        assert float(ps[0]) == s * inf and all(bool(torch.isnan(p).all()) for p in ps[1:])
        unsafe = s * _bits(0x7F7F8000)
        assert bool(torch.isfinite(unsafe).all())
        ps = pieces_of(unsafe, P)
        assert float(ps[0]) == s * inf and float(ps[1]) == -s * inf
        for b in (1.0, -0.3, 1e-30, 0.0):                                  # the kept products of the element cancel into NaN
            assert bool(torch.isnan(ps[0] * b + ps[1] * b).all())
        safe = s * _bits(0x7F7F7FFF)
        ps = pieces_of(safe, 3)
        assert all(bool(torch.isfinite(p).all()) for p in ps) and float(ps[0]) == s * float(_bits(0x7F7F0000))
        assert torch.equal(sum(p.double() for p in ps), safe.double())
    assert bool(torch.isnan(pieces_of(torch.tensor([float("nan")]), P)[0]).all())


def test_lo_piece_of_a_small_element_is_a_bf16_denormal():
    """below about 2^-117 the lo piece (|lo| <= 2^-9 |x|) falls under bf16's smallest normal 2^-126: hardware that flushes
    bf16 denormals loses it, at a cost of at most 2^-8 |x| (the bound of test_gemm_bound_on_small_magnitudes)"""
    x = torch.tensor([1.001953125 * 2.0 ** -118, 1.744140625 * 2.0 ** -120, 1.001953125 * 2.0 ** -116])   # lo = 2^-9 of the binade
    hi, lo = pieces_of(x, 2)
    assert torch.equal((hi + lo).double(), x.double())
    assert bool((lo[:2].abs() > 0).all()) and bool((lo[:2].abs() < 2.0 ** -126).all())      # denormal in bf16 and in fp32
    assert float(lo[2].abs()) >= 2.0 ** -126                                                  # 2^-116 * 2^-9: still normal
    assert bool((lo.abs() <= 2.0 ** -8 * x.abs()).all())
