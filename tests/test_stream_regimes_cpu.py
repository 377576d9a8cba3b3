"""The stream kernels' regimes without a GPU (tests/stream_regimes.py): the closed-form fp64 twins against autograd, the fp32
emulation of the LayerNorm kernels under the bounds that tests/test_stream_regimes_gpu.py applies to the kernels, on the
same inputs; the wrong variants rejected on the regimes named for them; and, from the twins alone, the share of every
output that stays finite (hence under a bound) in the non-finite cases."""
import pytest
import torch
import torch.nn.functional as F

from tests import stream_regimes as sr
from tests.test_stream_fp64_gpu import _up_ref, check, rejects

VARIANTS = sr.LN_VARIANTS


_ln_case = sr.ln_case


def _d(t):
    return None if t is None else t.double()


def test_closed_form_twin_is_autograd_of_layer_norm():
    x, gamma, beta, z, rs, dy, dadd = _ln_case(39, 96, "gated_rs", "base")
    K = sr.ln_K(39, 96, 1)
    t = sr.ln_twin(_d(x), _d(gamma), _d(beta), sr.EPS, K, _d(z), _d(rs), _d(dy))
    x64, g64, b64, z64 = (_d(v).requires_grad_() for v in (x, gamma, beta, z))
    y = F.layer_norm(x64, (96,), g64, b64, sr.EPS) * F.silu(z64) * _d(rs)[:, None]
    y.backward(_d(dy))
    for got, want in ((t["y"], y.detach()), (t["dx"], x64.grad), (t["dgamma"], g64.grad), (t["dbeta"], b64.grad), (t["dz"], z64.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_row_factor_tables():
    for n, rps, C in sr.LN_FACTOR:
        f = sr.factors(n)
        assert len(f) == n and f[(n - 1) // 2] == 0.0 and f[-1] != 0.0 and set(f) <= set(sr.FACTORS)
        assert all(a != b for a, b in zip(f, f[1:])) and f != f[1:] + f[:1]


def test_merge_grids_cover_every_residue():
    grids = [sr.merge_grid(*c) for c in sr.MERGE_CASES]
    assert {g % 8 for g in grids} == set(range(8)) and sum(g < 8 for g in grids) >= 6 and max(grids) > 16


@pytest.mark.parametrize("case", sr.LN_REGIME_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("regime", sr.LN_REGIMES)
def test_layernorm_emulation_stays_under_the_bounds(regime, case):
    """all four variants on every regime: y, mean, rstd, dx, dgamma, dbeta, dz of the two-pass fp32 emulation under the
    bounds (``second_order`` on every regime: it is nothing where the mean is small)"""
    rows, C = case
    K = sr.ln_K(rows, C, min(2048, -(-rows // 4)))
    for variant in VARIANTS:
        x, gamma, beta, z, rs, dy, dadd = _ln_case(rows, C, variant, regime)
        t = sr.ln_twin(_d(x), _d(gamma), _d(beta), sr.EPS, K, _d(z), _d(rs), _d(dy), _d(dadd), second_order=True)
        e = sr.ln_emulate(x, gamma, beta, sr.EPS, z, rs, dy, dadd)
        fam = f"ln emulation {regime}"
        for name, S in (("y", "S_y"), ("mean", "S_mean"), ("rstd", "S_rstd"), ("dx", "S_dx"), ("dgamma", "S_dg"), ("dbeta", "S_db")) + \
                ((("dz", "S_dz"),) if z is not None else ()):
            check(fam, e[name], t[name], t[S], K[name], f"{variant} {name}")
        if rs is not None:                                 # a zero factor: exact zeros
            dead = rs == 0
            assert bool(dead.any()) and bool((e["y"][dead] == 0).all()) and bool((e["dz"][dead] == 0).all()) and bool((e["dx"][dead] == 0).all())


@pytest.mark.parametrize("C", [96, 260, 1024])
def test_wrong_layernorm_variants_are_rejected(C):
    """one-pass variance on ``offset`` (where it is finite at all: NaN at offsets of 1e3 and above); eps outside the square
    root on ``constant`` and on the small end of ``wide``"""
    rows = 300
    K = sr.ln_K(rows, C, 75)
    x, gamma, beta, *_ = _ln_case(rows, C, "plain", "offset")
    t = sr.ln_twin(_d(x), _d(gamma), _d(beta), sr.EPS, K)
    bad = sr.ln_emulate(x, gamma, beta, sr.EPS, onepass=True)["y"]
    fin = torch.isfinite(bad).all(1)
    assert bool(fin.any()) and not bool(fin.all())
    assert sr.ratio(bad[fin], t["y"][fin], t["S_y"][fin], K["y"]) > 1.0
    # the kernel's stand-in must fail against the wrong fp64 variant too (what the GPU test asserts of the kernel)
    good = sr.ln_emulate(x, gamma, beta, sr.EPS)["y"]
    rejects(good[fin], bad[fin].double(), t["S_y"][fin], K["y"], "one-pass variance")
    for regime in ("constant", "wide"):
        x = sr.ln_regime(regime, rows, C, 900)
        if regime == "wide":
            x = x[:30]                                      # scales 2^-40 ... 2^-26: var << eps
        t = sr.ln_twin(_d(x), _d(gamma), _d(beta), sr.EPS, K)
        w = sr.ln_twin(_d(x), _d(gamma), _d(beta), sr.EPS, K, eps_out=True)
        good = sr.ln_emulate(x, gamma, beta, sr.EPS)
        rejects(good["rstd"], w["rstd"], t["S_rstd"], K["rstd"], f"eps outside the sqrt ({regime}, rstd)")
        if regime == "wide":
            rejects(good["y"], w["y"], t["S_y"], K["y"], "eps outside the sqrt (wide, y)")
        assert sr.ratio(sr.ln_emulate(x, gamma, beta, sr.EPS, eps_out=True)["rstd"], t["rstd"], t["S_rstd"], K["rstd"]) > 1.0


@pytest.mark.parametrize("C", [96, 260, 1024])
@pytest.mark.parametrize("variant", ["gated", "gated_rs"])
def test_saturated_gates_stay_under_the_extended_bounds(variant, C):
    """gates of +-20 ... +-200: the emulation under the bounds with the argument-error and underflow terms in S"""
    rows = 300
    K = sr.ln_K(rows, C, 75)
    x, gamma, beta, z, rs, dy, dadd = _ln_case(rows, C, variant, "base", gate="saturated")
    assert {abs(float(v)) for v in z[:, 1::4].unique()} == set(sr.GATES)
    t = sr.ln_twin(_d(x), _d(gamma), _d(beta), sr.EPS, K, _d(z), _d(rs), _d(dy), saturated=True)
    e = sr.ln_emulate(x, gamma, beta, sr.EPS, z, rs, dy)
    for name, S in (("y", "S_y"), ("dx", "S_dx"), ("dgamma", "S_dg"), ("dbeta", "S_db"), ("dz", "S_dz")):
        r = check(f"ln emulation saturated", e[name], t[name], t[S], K[name], f"{variant} {name}")
        print(f"saturated {variant} C={C} {name}: {r:.3g}")
    # a sigmoid without saturation handling (1 - sigma formed as exp(-z) sigma, overflowing) is not what the kernel does:
    # a wrong variant that clamps the gate at +-60 must be rejected
    zc = z.clamp(-60, 60)
    w = sr.ln_twin(_d(x), _d(gamma), _d(beta), sr.EPS, K, _d(zc), _d(rs), _d(dy))
    rejects(e["y"], w["y"], t["S_y"], K["y"], "gate clamped at +-60")
    # silu' taken as sigma alone (the z (1 - sigma) term dropped): seen at the N(0, 1) gates
    a = _d(dy) * (_d(rs)[:, None] if rs is not None else 1.0)
    rejects(e["dz"], a * t["n"] * torch.sigmoid(_d(z)), t["S_dz"], K["dz"], "silu' without its z (1 - sigma) term")
    # the negative side, on the rows' saturated NEGATIVE gates alone: sigma flushed to zero below -15 (y and dz are 2e-9 of
    # their factors at z = -20 and the bound is relative to that), and the clamp at -60 (seen from -88 on)
    live = (_d(rs) != 0)[:, None] if rs is not None else torch.ones(rows, 1, dtype=torch.bool)
    neg = (z <= -20.0) & live
    for name, S in (("y", "S_y"), ("dz", "S_dz")):
        rejects(e[name][neg], sr.flushed(_d(z), t[name])[neg], t[S][neg], K[name], f"{name}: sigma flushed to zero below -15")
        only20 = (z == -20.0) & live
        rejects(e[name][only20], sr.flushed(_d(z), t[name])[only20], t[S][only20], K[name], f"{name}: sigma flushed to zero at z = -20")
    far = (z <= -88.0) & live
    rejects(e["y"][far], w["y"][far], t["S_y"][far], K["y"], "gate clamped at -60, negative gates alone")


def test_upsample_adjoint_twin_is_autograd_of_the_reference():
    for B, H, W, C in sr.UP_CASES:
        g = torch.randn(B, 2 * H, 2 * W, C, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        x = torch.zeros(B, H, W, C, dtype=torch.float64, requires_grad=True)
        _up_ref(x).backward(g)
        assert float((sr.up_adjoint(g) - x.grad).abs().max()) <= 1e-14


@pytest.mark.parametrize("case", [(1, 3, 3, 4), (1, 2, 5, 12), (2, 1, 7, 8), (2, 9, 11, 4)], ids=str)
def test_upsample_poison_reaches_exactly_its_readers(case):
    """a NaN pixel makes exactly ``up_readers`` non-finite in the twins, and at least 90 % of either output stays finite at
    the (2, 9, 11, 4) shape the GPU test poisons"""
    B, H, W, C = case
    for y, x in ((0, 0), (H - 1, W - 1), (H // 2, W // 2), (0, min(1, W - 1))):
        fwd, _ = sr.up_readers(H, W, y, x)
        a = torch.randn(B, H, W, C, dtype=torch.float64)
        a[0, y, x, 1] = sr.NAN
        bad = ~torch.isfinite(_up_ref(a))
        want = torch.zeros_like(bad)
        for oy, ox in fwd:
            want[0, oy, ox, 1] = True
        assert torch.equal(bad, want)
        g = torch.randn(B, 2 * H, 2 * W, C, dtype=torch.float64)
        g[0, 2 * y, 2 * x, 1] = sr.NAN
        _, adj = sr.up_readers(H, W, 2 * y, 2 * x)
        bad = ~torch.isfinite(sr.up_adjoint(g))
        want = torch.zeros_like(bad)
        for iy, ix in adj:
            want[0, iy, ix, 1] = True
        assert torch.equal(bad, want)
        if case == (2, 9, 11, 4):
            assert float((~bad).double().mean()) >= 0.9 and len(fwd) * 10 <= B * 4 * H * W * C


@pytest.mark.parametrize("case", [(300, 260), (9003, 96), (300, 1024)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_layernorm_poison_stays_in_its_rows(case):
    """from the twin alone: poisoned x rows / one gate element / one dy element leave >= 90 % of every row-wise output and
    of dbeta finite (dgamma sums xhat of every row into every column: a poisoned x row takes all of it)"""
    rows, C = case
    K = sr.ln_K(rows, C, 75)
    x, gamma, beta, z, rs, dy, dadd = _ln_case(rows, C, "gated_rs", "base")
    prow = sr.ln_poison_rows(rows)
    one = prow[len(prow) // 2]
    assert 3 <= len(prow) <= 12 and all(sr.ln_last_row_of_wave0(rows, 4 * min(-(-rows // 4), 256 * occ)) in prow for occ in range(1, 9))
    for target in ("x", "gate", "dy"):
        for v in sr.POISONS:
            xx, zz, dd = x.clone(), z.clone(), dy.clone()
            if target == "x":
                xx[prow, 5] = v
            else:
                (zz if target == "gate" else dd)[one, 5] = v
            t = sr.ln_twin(_d(xx), _d(gamma), _d(beta), sr.EPS, K, _d(zz), _d(rs), _d(dd))
            for name in ("y", "mean", "rstd", "dx", "dz", "dbeta"):
                share = float(torch.isfinite(t[name]).double().mean())
                assert share >= 0.9, (target, v, name, share)
            bad_rows = ~torch.isfinite(t["dx"]).all(1)
            assert sorted(torch.nonzero(bad_rows)[:, 0].tolist()) == (sorted(prow) if target == "x" else [one])
            if target == "x":
                assert bool(torch.isfinite(t["dbeta"]).all()) and not bool(torch.isfinite(t["dgamma"]).any())


def test_plane_inputs_plant_what_they_say():
    for hw in sr.PLANE_HW:
        x = sr.plane_inputs(5, hw, ("tied", "constant", "last", "neg_inf", "pos_inf"), 3)
        mx = x.max(1).values
        cnt = (x == mx[:, None]).sum(1).tolist()
        assert cnt == [min(2, hw), hw, 1, hw, min(2, hw)]
        assert int(x[2].argmax()) == hw - 1 and float(mx[3]) == -sr.INF and float(mx[4]) == sr.INF


@pytest.mark.parametrize("case", sr.DW_CASES, ids=str)
def test_dwconv_saturated_emulation_stays_under_the_extended_bounds(case):
    """pre-activations of +-20 ... +-200 through the bias and an input of one sign per plane: out2, gpre, dx, dweight, dbias
    of the fp32 emulation under the bounds with the argument-error and underflow terms; the pre-activation clamped at +-60
    is rejected; after ``dw_rounds`` runs every value has been a plane's interior pre-activation"""
    seen = set()
    for rnd in range(sr.dw_rounds(case)):
        x, w, b, g2, v = sr.dw_saturated_inputs(case, rnd, 910)
        K = sr.dw_K(case, True)
        t = sr.dw_twin(_d(x), _d(w), _d(b), _d(g2), 2, K, saturated=True)
        e = sr.dw_emulate(x, w, b, g2, 2)
        B, d, H, W = case
        mid = t["pre"][:, :, H // 2, W // 2]
        assert float(((mid - v.double()).abs() / v.double().abs()).max()) < 2e-3 and bool((x.flatten(2).sign().std(2) == 0).all())
        seen |= set(v.flatten().tolist())
        for name in ("out2", "gpre", "dx", "dweight", "dbias"):
            check("dwconv emulation saturated", e[name], t[name], t["S_" + name], K[name], f"{case} round {rnd} {name}")
        if float(v.abs().max()) > 60:
            rejects(e["out2"], sr.dw_twin(_d(x), _d(w), _d(b), _d(g2), 2, K, clamp=60.0)["out2"], t["S_out2"], K["out2"], "pre clamped at +-60")
    assert seen == set(sr.DW_VALUES)


@pytest.mark.parametrize("case", sr.DW_CASES, ids=str)
def test_dwconv_poison_reaches_exactly_its_neighbourhood(case):
    """from the twin alone: a non-finite input pixel makes its 3 x 3 neighbourhood of out2 (both memory orders) and of gpre
    and the 5 x 5 one of dx non-finite, with the sums of its channel; at least 90 % of out2, gpre and dx stay finite (the
    per-channel sums lose the poisoned channel, one of d)"""
    B, d, H, W = case
    K = sr.dw_K(case, True)
    for h, w_ in ((0, 0), (H - 1, W // 2), (H // 2, W // 2)):
        for v in sr.POISONS:
            x, w, b, g2 = sr.dw_inputs(case, 920)
            x[B - 1, 1, h, w_] = v
            t = sr.dw_twin(_d(x), _d(w), _d(b), _d(g2), 2, K)
            near, far = sr.dw_neighbours(H, W, h, w_), sr.dw_neighbours(H, W, h, w_, 2)
            bad = ~torch.isfinite(t["gpre"])
            assert int(bad.sum()) == len(near) and all(bool(bad[B - 1, 1, a, c]) for a, c in near)
            assert int((~torch.isfinite(t["out2"])).sum()) == 2 * len(near)
            bad = ~torch.isfinite(t["dx"])
            assert int(bad.sum()) == len(far) and all(bool(bad[B - 1, 1, a, c]) for a, c in far)
            for name in ("out2", "gpre", "dx"):
                assert float(torch.isfinite(t[name]).double().mean()) >= 0.9, (name, case)
            for name in ("dweight", "dbias"):
                fin = torch.isfinite(t[name])
                assert not bool(fin[1].any()) and bool(fin[[c for c in range(d) if c != 1]].all())


@pytest.mark.parametrize("hw", [1000, 1001])
def test_plane_poison_leaves_22_planes_of_24(hw):
    """from the twin alone: one poisoned pixel of x (plane 5) and one of g (plane 17) leave at least 90 % of mean, max,
    scale, dot and gate_bwd finite, and touch those two planes alone"""
    for v in sr.POISONS:
        t = sr.plane_twin(*sr.plane_poison_inputs(hw, v, 66))
        for name in ("mean", "max", "scale", "dot", "gate_bwd"):
            fin = torch.isfinite(t[name])
            assert float(fin.double().mean()) >= 0.9, (name, v)
            rows = fin.reshape(sr.PLANE_POISON_P, -1).all(1)
            assert bool(rows[[p for p in range(sr.PLANE_POISON_P) if p not in (5, 17)]].all()), (name, v)
        assert not bool(torch.isfinite(t["mean"][5])) and not bool(torch.isfinite(t["dot"][17])) and not bool(torch.isfinite(t["dot"][5]))
        assert bool(torch.isfinite(t["mean"][17])) and int((~torch.isfinite(t["gate_bwd"])).sum()) == 1


def test_layout_and_colscale_poison_shares():
    """from the twins alone: at least 90 % of the outputs of merge, pair_sum_add and both colscale outputs stay finite"""
    for v in sr.POISONS:
        (B, d, H, W), e4, en = sr.MERGE_POISON
        p4, nh = torch.randn(B, 4, d, H * W), torch.randn(B, H, W, d)
        p4[(e4[0], e4[1], e4[2], e4[3])] = v
        ref = sr.merge_ref(p4, nh)[0]
        assert int((~torch.isfinite(ref)).sum()) == 1
        for no, inner, _ in sr.PAIR_POISON:
            src, acc = sr.pair_poison_inputs(no, inner, v, 41)
            out = acc.double() + src.double().sum(1)
            assert int((~torch.isfinite(out)).sum()) == 2 and float(torch.isfinite(out).double().mean()) >= 0.9
        for C in (96, 516):
            dy, x, s = sr.colscale_poison_inputs(C, v, 71)
            dx, ds = dy.double() * s.double(), (dy.double() * x.double()).sum(0)
            assert int((~torch.isfinite(dx)).sum()) == 1 and int((~torch.isfinite(ds)).sum()) == 2
            assert float(torch.isfinite(ds).double().mean()) >= 0.9
