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
