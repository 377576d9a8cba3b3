"""The fp64 scan reference and its bounds (tests/scan_fp64_ref.py), checked without a GPU: the reference against the C
oracle, the committed golden vectors and float64 autograd of a literal loop; honest fp32 implementations (the C oracle's
fp32 form, a sequential fp32 torch recurrence with its backward) INSIDE every bound on every regime; plausible defects
OUTSIDE it by a factor of three or more, the fp32 stand-in playing the kernel; and the planner's kernel family for every
case of tests/test_scan_fp64_gpu.py."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from tests import scan_fp64_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias"]
# one small problem per regime: two images, two groups (the second reversed), a length past the 640-checkpoint
SMALL = dict(batch=2, KD=8, L=700, N=8, G=2)
MASK = 0b10


def serial_constants(batch, KD, L, G):
    """the fp32 stand-in: a sequential recurrence (k: A * delta 1, nothing summed; no scan network: c_0 = hand-over 2),
    torch sums taken at their worst depth (rows of a group; batch x L positions)"""
    return R.Constants(k=2.5, c_0=2.0, K_rows=float(KD // G), K_row=float(batch * L))


def flip_groups(t, G, mask):
    """the groups of ``mask`` of a (b, G * rows, L) or (b, G, N, L) tensor reversed along the sequence"""
    t = t.clone()
    v = t.view(t.shape[0], G, -1, t.shape[-1])
    for g in range(G):
        if (mask >> g) & 1:
            v[:, g] = v[:, g].flip(-1)
    return t


def standin(args, mask=0, dtype=torch.float32, naive_softplus=False):
    """forward and the seven gradients by a literal sequential recurrence in ``dtype`` (float32: the stand-in for a
    kernel; float64: the literal loop the reference's gradients are checked against)"""
    u, delta, A, B, C, D, bias, dout, softplus = args
    G, N = B.shape[1], B.shape[2]
    c = lambda t: None if t is None else t.to(dtype)
    u, delta, B, C, dout = (flip_groups(c(t), G, mask) for t in (u, delta, B, C, dout))
    A, D, bias = c(A), c(D), c(bias)
    batch, KD, L = delta.shape
    rows = KD // G
    Bx, Cx = B.repeat_interleave(rows, 1), C.repeat_interleave(rows, 1)              # (b, KD, N, L)
    raw = delta + (bias[None, :, None] if bias is not None else 0)
    if softplus:
        if naive_softplus:
            dl = torch.log(1 + torch.exp(raw))
        else:
            dl = torch.where(raw > 20, raw, torch.nn.functional.softplus(torch.clamp(raw, max=20.0), threshold=1e9))
        sig = torch.where(raw > 20, torch.ones_like(raw), torch.sigmoid(raw))
    else:
        dl, sig = raw, torch.ones_like(raw)
    a = torch.exp(dl[:, :, None, :] * A[None, :, :, None])                             # (b, KD, N, L)
    w = (dl * u)[:, :, None, :] * Bx
    xs = torch.zeros(batch, KD, N, L + 1, dtype=dtype)
    for t in range(L):
        xs[..., t + 1] = a[..., t] * xs[..., t] + w[..., t]
    out = (Cx * xs[..., 1:]).sum(2) + D[None, :, None] * u
    lam = torch.zeros(batch, KD, N, L + 1, dtype=dtype)
    src = dout[:, :, None, :] * Cx
    for t in range(L - 1, -1, -1):
        lam[..., t] = src[..., t] + (a[..., t + 1] * lam[..., t + 1] if t + 1 < L else 0)
    lam = lam[..., :L]
    sB = (Bx * lam).sum(2)
    du = dl * sB + D[None, :, None] * dout
    ax = a * xs[..., :L]
    dd = (u * sB + (A[None, :, :, None] * ax * lam).sum(2)) * sig
    dA = (dl[:, :, None, :] * ax * lam).sum((0, 3))
    dB = ((dl * u)[:, :, None, :] * lam).view(batch, G, rows, N, L).sum(2)
    dC = (dout[:, :, None, :] * xs[..., 1:]).view(batch, G, rows, N, L).sum(2)
    dD = (dout * u).sum((0, 2))
    db = dd.sum((0, 2))
    f = lambda t: flip_groups(t, G, mask)
    return {"out": f(out), "du": f(du), "ddelta": f(dd), "dA": dA, "dB": f(dB), "dC": f(dC), "dD": dD, "ddelta_bias": db}


def problem(regime, seed=1, **kw):
    return R.make(regime, SMALL["batch"], SMALL["KD"], SMALL["L"], SMALL["N"], SMALL["G"], seed=seed, **kw)


def ref_of(args, wrong=None, wrong_at=0, mask=MASK):
    cs = serial_constants(SMALL["batch"], SMALL["KD"], SMALL["L"], SMALL["G"])
    ref, S, _ = R.reference(*args[:8], args[8], cs, rev_mask=mask, wrong=wrong, wrong_at=wrong_at)
    return ref, S


def outputs_of(args):
    return [n for n in R.OUTPUTS if not (n == "ddelta_bias" and args[6] is None)]


# ------------------------------------------------------------------------------------------- the reference is right
@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_reference_agrees_with_the_c_oracle(regime):
    """forward (acc64) and backward (always double) of oracle/scan_oracle.c, whose outputs are fp32: to fp32 output
    rounding, |oracle - ref| <= U (1.01 |ref| + 1e-6 S) + 2^-149 (the oracle forms a x_{t-1} as x_t - w_t)"""
    from oracle import scan_oracle as so
    args = problem(regime)
    u, delta, A, B, C, D, bias, dout, softplus = args
    ref, S = ref_of(args, mask=0)
    got = {"out": so.selective_scan_oracle(u, delta, A, B, C, D, bias, softplus, acc64=True)}
    got.update(zip(NAMES, so.selective_scan_oracle_bwd(u, delta, A, B, C, D, bias, dout, softplus)))
    for name in outputs_of(args):
        err = (got[name].double() - ref[name]).abs()
        tol = R.U * (1.01 * ref[name].abs() + 1e-6 * S[name]) + 2.0 ** -149
        assert bool((err <= tol).all()), f"{regime} {name}: {float((err / tol).max()):.3g} of the rounding of an fp32 output"


FILES = sorted(glob.glob(os.path.join(GOLDEN, "scan_*.npz")))


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p)[5:-4] for p in FILES])
def test_reference_agrees_with_the_golden_vectors(path):
    """the committed outputs of the reference project's own code, at the tolerances tests/test_scan_gpu.py holds the
    kernels to (the vectors were produced in the dtype of the case: its tolerances apply)"""
    import ast
    z = np.load(path, allow_pickle=False)
    meta = ast.literal_eval(str(z["meta"]))
    dt = getattr(torch, meta["dtype"])
    t = {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}
    rtol, atol = {torch.float32: (6e-4, 2e-3), torch.float16: (3e-3, 5e-3)}.get(dt, (3e-2, 5e-2))
    g = lambda k: t.get("in_" + k)
    B, C = g("B"), g("C")
    B4, C4 = (B if B.dim() == 4 else B[:, None]), (C if C.dim() == 4 else C[:, None])
    batch, KD, L = g("delta").shape
    cs = serial_constants(batch, KD, L, B4.shape[1])
    ref, _, _ = R.reference(g("u"), g("delta"), g("A"), B4, C4, g("D"), g("delta_bias"), g("dout"), meta["softplus"], cs)
    close = lambda a, b, rt, at, what: torch.testing.assert_close(a.float(), b.float(), rtol=rt, atol=at, msg=lambda m: f"{what}: {m}")
    close(ref["out"], t["out"], rtol, atol, "out")
    close(ref["du"], t["grad_u"], 2 * rtol, 2 * atol, "du")
    close(ref["ddelta"], t["grad_delta"], 5 * rtol, 10 * atol, "ddelta")
    close(ref["dB"].reshape(B.shape), t["grad_B"], rtol, atol, "dB")
    close(ref["dC"].reshape(C.shape), t["grad_C"], rtol, atol, "dC")
    close(ref["dA"], t["grad_A"], 1e-3, 5e-3, "dA")
    if g("D") is not None:
        close(ref["dD"], t["grad_D"], 1e-3, 1e-3, "dD")
    if g("delta_bias") is not None:
        close(ref["ddelta_bias"], t["grad_delta_bias"], 1e-3, 1e-3, "ddelta_bias")


@pytest.mark.parametrize("softplus", [True, False], ids=["softplus", "plain"])
def test_reference_gradients_equal_float64_autograd_of_a_literal_loop(softplus):
    g = torch.Generator().manual_seed(5)
    batch, KD, L, N, G = 2, 6, 37, 4, 2
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    leaves = [r(batch, KD, L), 0.5 * r(batch, KD, L), -torch.rand(KD, N, generator=g, dtype=torch.float64) - 0.2,
              r(batch, G, N, L), r(batch, G, N, L), r(KD), 0.3 * r(KD)]
    for t in leaves:
        t.requires_grad_()
    u, delta, A, B, C, D, bias = leaves
    dout = r(batch, KD, L)
    rows = KD // G
    dl = delta + bias[None, :, None]
    if softplus:
        dl = torch.nn.functional.softplus(dl)
    x = torch.zeros(batch, KD, N, dtype=torch.float64)
    ys = []
    for t in range(L):
        Bt, Ct = B[..., t].repeat_interleave(rows, 1), C[..., t].repeat_interleave(rows, 1)
        x = torch.exp(dl[:, :, t, None] * A[None]) * x + (dl[:, :, t] * u[:, :, t])[..., None] * Bt
        ys.append((x * Ct).sum(-1) + D[None] * u[:, :, t])
    out = torch.stack(ys, -1)
    grads = torch.autograd.grad(out, leaves, dout)
    ref, _, _ = R.reference(*[t.detach() for t in leaves], dout, softplus, serial_constants(batch, KD, L, G))
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert rel(ref["out"], out.detach()) <= 1e-10
    for name, gr in zip(NAMES, grads):
        assert rel(ref[name], gr) <= 1e-10, f"{name}: {rel(ref[name], gr):.3g}"


def test_scans_equal_the_loop_and_row_blocks_do_not_matter():
    g = torch.Generator().manual_seed(2)
    for L in (77, 128, 301):                             # doubling; blocked, whole blocks; blocked with a padded last block
        a, w = torch.rand(3, 5, L, generator=g, dtype=torch.float64) * 1.2, torch.randn(3, 5, L, generator=g, dtype=torch.float64)
        x, acc = torch.zeros(3, 5, dtype=torch.float64), []
        for t in range(L):
            x = a[..., t] * x + w[..., t]
            acc.append(x)
        keep = (a.clone(), w.clone())
        torch.testing.assert_close(R.lin_scan(a, [w])[0], torch.stack(acc, -1), rtol=1e-12, atol=1e-12)
        assert torch.equal(a, keep[0]) and torch.equal(w, keep[1])
        y, acc = torch.zeros(3, 5, dtype=torch.float64), []
        for t in range(L - 1, -1, -1):
            y = a[..., t] * y + w[..., t]
            acc.append(y)
        torch.testing.assert_close(R.lin_scan_rev(a, [w])[0], torch.stack(acc[::-1], -1), rtol=1e-12, atol=1e-12)
    args = problem("grid")
    cs = serial_constants(SMALL["batch"], SMALL["KD"], SMALL["L"], SMALL["G"])
    whole = R.reference(*args[:8], args[8], cs, rev_mask=MASK)
    parts = R.reference(*args[:8], args[8], cs, rev_mask=MASK, elems=3 * SMALL["N"] * SMALL["L"])       # 3 of the 4 rows at a time
    for d0, d1 in zip(whole, parts):
        for k in d0:
            torch.testing.assert_close(d1[k], d0[k], rtol=1e-12, atol=1e-300)


# ----------------------------------------------------------------------------- honest fp32 is inside, every regime
@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_fp32_implementations_stay_inside_every_bound(regime, capsys):
    from oracle import scan_oracle as so
    args = problem(regime)
    ref, S = ref_of(args)
    got = standin(args, MASK)
    ratios = {n: R.ratio(got[n], ref[n], S[n]) for n in outputs_of(args)}
    u, delta, A, B, C, D, bias, dout, softplus = args
    G = SMALL["G"]
    fo = flip_groups(so.selective_scan_oracle(flip_groups(u, G, MASK), flip_groups(delta, G, MASK), A, flip_groups(B, G, MASK),
                                              flip_groups(C, G, MASK), D, bias, softplus, acc64=False), G, MASK)
    ratios["out (C oracle, fp32)"] = R.ratio(fo, ref["out"], S["out"])
    with capsys.disabled():
        print(f"\n  {regime:12s} fp32 stand-in err / (U S): " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for v in ref.values():
        assert bool(torch.isfinite(v.float()).all()), "the regime leaves the fp32 range"
    assert all(v <= 1.0 for v in ratios.values()), ratios


# ------------------------------------------------------------------------------------------- defects are outside
# (wrong variant of the reference, regime, the outputs that must see it by a factor >= 3, single = no other output may)
CONTROLS = [
    ("bf16_decay", "init", ("out", "du", "dC"), False),
    ("exp_1e-5", "long_memory", ("out", "du", "dB", "dC"), False),
    ("drop_carry", "long_memory", ("out", "dC"), False),
    ("threshold10", "threshold", ("out",), False),
    ("sigmoid1_10", "threshold", ("ddelta",), True),
    ("adjoint_at", "init", ("du", "ddelta", "dA", "dB"), False),
    ("rev_skip_first", "init", ("out", "dC"), False),
    ("dB_last_row", "init", ("dB",), True),
    ("dC_last_row", "init", ("dC",), True),
    ("dA_last_image", "init", ("dA",), True),
    ("out_D", "init", ("out",), True),
    ("du_D", "init", ("du",), True),
]


@pytest.mark.parametrize("wrong,regime,sees,single", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_defects_exceed_the_bound_threefold(wrong, regime, sees, single):
    args = problem(regime)
    got = standin(args, MASK)
    bad, S = ref_of(args, wrong=wrong, wrong_at=640)
    ratios = {n: R.ratio(got[n], bad[n], S[n]) for n in outputs_of(args)}
    print(f"{wrong} on {regime}: " + "  ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    for n in sees:
        assert ratios[n] >= 3.0, f"{wrong} on {regime}: {n} at {ratios[n]:.3g} of its bound -- the bound cannot see it"
    if single:
        for n, v in ratios.items():
            assert n in sees or n == "ddelta_bias" or v <= 1.0, f"{wrong}: {n} moved too ({v:.3g})"


def test_softplus_without_log1p_exceeds_the_bound_threefold():
    """softplus as fp32 log(1 + exp(x)) on a variant of init with dt down to 1e-4 (on init itself: too close to serve)"""
    args = problem("init", dt_lo=1e-4)
    ref, S = ref_of(args)
    got = standin(args, MASK, naive_softplus=True)
    assert R.ratio(got["out"], ref["out"], S["out"]) >= 3.0
    assert R.ratio(standin(args, MASK)["out"], ref["out"], S["out"]) <= 1.0


def test_non_finite_output_fails():
    args = problem("grid")
    ref, S = ref_of(args)
    got = standin(args, MASK)["out"]
    got[1, 3, 17] = float("nan")
    assert R.ratio(got, ref["out"], S["out"]) == float("inf")


# ------------------------------------------------------------------------------------------- the planner's choice
def test_planner_picks_the_intended_family_for_every_gpu_case():
    from sigma_amd import _capi
    from tests.test_deterministic_cpu import bwd_params, family_of, fwd_family_of, segments_of
    from tests.test_scan_fp64_gpu import CASES, IO, plans
    lib = _capi.load()
    for case in CASES:
        name, batch, KD, L, N, G, mask, ush, pitch, dtype, fwd_fam, fwd_seg, bwd_fam, bwd_seg = case
        fp, bp = plans(lib, batch, KD, L, N, G, mask, ush, pitch, IO[dtype])
        assert fwd_family_of(fp) == fwd_fam, (name, fp)
        assert (fwd_fam == "Fwdr" and fp[4] > 1) == fwd_seg, (name, fp)
        assert family_of(bp) == bwd_fam, (name, bp)
        assert (segments_of(bp) > 1) == bwd_seg, (name, bp)
        det = (ctypes.c_int32 * 6)()
        assert lib.sigma_scan_bwd_plan(ctypes.byref(bwd_params(batch, KD, L, N, G, mask, ush, pitch, IO[dtype],
                                                               _capi.SIGMA_SCAN_BWD_DETERMINISTIC)), ctypes.byref(det)) == 0
        assert list(det) == bp, name


# ------------------------------------------------------------------------- the footprint of one non-finite element
# tests/scan_footprint.py: the rule == the fp64 reference == a literal fp64 loop, every operand, both directions
from tests import scan_footprint as F  # noqa: E402

TINY_DIMS = (2, 8, 37, 4, 4)                        # batch, KD, L, N, G: groups 1 and 3 reversed, u / dout shared by pairs
TINY_KW = dict(rev_mask=0b1010, u_gshift=1, dout_gshift=1)
PLANT_KINDS = [(op, v) for op in F.SEQ_OPERANDS for v in (F.NAN, F.INF)] + [(op, F.NAN) for op in F.ROW_OPERANDS]
KIND_IDS = [f"{op}-{'nan' if v != v else 'inf'}" for op, v in PLANT_KINDS]


def tiny_problem(regime="init"):
    batch, KD, L, N, G = TINY_DIMS
    return R.make(regime, batch, KD, L, N, G, ush=1, seed=3)


def tiny_plants(op, value):
    """a plant per direction at the first, the second, an inner and the last position (row operands: one row each way)"""
    batch, KD, L, N, G = TINY_DIMS
    rows = KD // G
    if op in F.ROW_OPERANDS:
        return [F.Plant(op, ((g * rows + 1, 2) if op == "A" else (g * rows + 1,)), value) for g in (0, 1)]
    out = []
    for t in (0, 1, L // 2, L - 1):
        if op in ("u", "dout"):
            out.append(F.Plant(op, (1, 1, t), value))                     # feeds groups 0 and 1: both directions at once
        for g in (0, 1) if op not in ("u", "dout") else ():
            out.append(F.Plant(op, (1, g * rows + 1, t) if op == "delta" else (0, g, 2, t), value))
    return out


def tiny_reference(args, **kw):
    batch, KD, L, N, G = TINY_DIMS
    return R.reference(*args[:8], args[8], serial_constants(batch, KD, L, G), finite=False, **TINY_KW, **kw)


def literal_loop(args):
    """the literal sequential fp64 loop of ``standin`` on the same operands (shared u / dout rows written out per group)"""
    batch, KD, L, N, G = TINY_DIMS
    rows = KD // G
    src = torch.cat([torch.arange(rows) + (g >> 1) * rows for g in range(G)])
    args = list(args)
    args[0], args[7] = args[0][:, src], args[7][:, src]
    return standin(args, TINY_KW["rev_mask"], dtype=torch.float64)


@pytest.mark.parametrize("op,value", PLANT_KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("regime", ["init", "neg_delta"])            # softplus with a bias; plain delta without one
def test_footprint_rule_equals_the_reference_and_a_literal_loop(regime, op, value):
    """the non-finite set of the fp64 reference on operands holding ONE plant EQUALS the rule's mask, for every operand,
    NaN and +inf, forward and reversed rows, first / inner / last position -- no exception; and so does the set of a
    literal sequential fp64 loop (the doubling scan of lin_scan does not smear it).  Finite against non-finite only."""
    args = tiny_problem(regime)
    if args[F.ARG_INDEX[op]] is None:
        assert regime == "neg_delta" and op == "delta_bias"         # the regime has no bias: nothing to plant in
        return
    for plant in tiny_plants(op, value):
        want = F.footprint(plant, TINY_DIMS, softplus=args[8], **TINY_KW)
        planted = F.plant_into(args, [plant])
        got = F.non_finite_sets(tiny_reference(planted)[0])
        loop = F.non_finite_sets(literal_loop(planted))
        for name in outputs_of(args):
            show = lambda m: m.nonzero().tolist()[:8]
            assert torch.equal(got[name], want[name]), f"{plant} {name}: reference {show(got[name])} rule {show(want[name])}"
            assert torch.equal(loop[name], want[name]), f"{plant} {name}: loop {show(loop[name])} rule {show(want[name])}"
        for name in ("out", "du", "ddelta", "dB", "dC"):            # what the GPU test asserts per plant: not vacuous
            assert bool(want[name].any()) == (name in F.reached(plant, TINY_DIMS, **TINY_KW)), (plant, name)
            assert not bool(want[name].all())


def test_footprint_launch_plans_cover_every_position_in_disjoint_cones():
    """``launches``: every position both ways, every launch's cones pairwise disjoint (the GPU cases' group layout)"""
    dims, kw = (2, 32, 700, 4, 4), dict(rev_mask=0b1010, u_gshift=1, dout_gshift=1)
    ts = F.positions(700, segment_starts=(352,))
    assert ts == [0, 1, 2, 3, 16, 160, 352, 640, 699]
    for op, value in PLANT_KINDS:
        plan = F.launches(op, value, dims, 0b1010, 1, 1, ts)
        seen = set()
        for plants in plan:
            cones = [F.footprint(p, dims, **kw) for p in plants]
            assert F.disjoint(cones), (op, plants)
            for p in plants:
                seen |= {(t, rev) for _, _, _, rev, t, _ in F.rows_of(p, dims, **kw)}
        want = {(t, d) for t in ts for d in (False, True)} if op in F.SEQ_OPERANDS else {(None, False), (None, True)}
        assert seen == want, (op, sorted(want - seen))
        assert len(plan) <= 5, (op, len(plan))


# (control, what the checker must report): only reference code runs here -- the planted reference plays the kernel
FOOTPRINT_CONTROLS = ["cone_shifted_one_tile", "dB_cone_whole_group_row", "lost_nan"]


@pytest.mark.parametrize("control", FOOTPRINT_CONTROLS)
def test_footprint_checker_fails_wrong_cones_and_a_lost_nan(control):
    """the checker of the GPU test (F.check) on the fp64 reference's own planted outputs: clean against the true rule;
    a cone shifted by one 16-tile, a dB cone widened to the whole row of the group, and a plant replaced by zero (a NaN
    that got lost) must each be reported"""
    args = tiny_problem("init")
    plant = F.Plant("u", (1, 1, 18), F.NAN)
    clean, S, _ = tiny_reference(args)
    cones, owns = F.footprint(plant, TINY_DIMS, **TINY_KW), F.own(plant, TINY_DIMS, 16, **TINY_KW)
    got, _, _ = tiny_reference(F.plant_into(args, [plant]))
    assert F.check(got, cones, owns, clean, S) == ([], {})
    if control == "cone_shifted_one_tile":
        cones = F.footprint(F.Plant("u", (1, 1, 18 - 16), F.NAN), TINY_DIMS, **TINY_KW)
        expect = ("out: ", "dB: ", "dC: ")
    elif control == "dB_cone_whole_group_row":
        cones = dict(cones, dB=cones["dB"].clone())
        cones["dB"][1, 0] = True
        expect = ("dB: ",)
    else:
        got, _, _ = tiny_reference(F.plant_into(args, [F.Plant("u", (1, 1, 18), 0.0)]))
        expect = ("out: ", "ddelta: ", "dB: ", "dC: ", "dA: ", "dD: ")
    failures, _ = F.check(got, cones, owns, clean, S)
    for e in expect:
        assert any(f.startswith(e) for f in failures), (control, e, failures)
    # a stray NaN in another row is a failure whatever the table allows; inside the own row only the table excuses it
    cones, got = F.footprint(plant, TINY_DIMS, **TINY_KW), tiny_reference(F.plant_into(args, [plant]))[0]
    got["du"][0, 5, 3] = float("nan")
    assert any(f.startswith("du: ") for f in F.check(got, cones, owns, clean, S, excused={"du": owns["du"]})[0])
    got["du"][0, 5, 3] = clean["du"][0, 5, 3]
    got["du"][1, 1, 3] = float("nan")
    assert F.check(got, cones, owns, clean, S, excused={"du": owns["du"]}) == ([], {"du": 1})
    assert any(f.startswith("du: ") for f in F.check(got, cones, owns, clean, S)[0])
