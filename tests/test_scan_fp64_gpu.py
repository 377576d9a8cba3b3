"""The selective-scan kernels against the fp64 reference of tests/scan_fp64_ref.py under its derived bound
|got - ref| <= U S, every kernel family on every value regime it takes; run with -m gpu.

Every case goes through the binding (fwd_ext / bwd_ext) under ``recording()`` and asserts its census keys, so that it
cannot pass on another kernel than it names; the backward runs in the default and in the deterministic form.  Every
element of every output is held to its bound (a non-finite element fails); nothing is masked, and there is no floor
beyond S.  Sharpness is shown on the kernels' own outputs: plausible wrong fp64 variants that they must FAIL.  Guard
bands: through the C ABI the outputs land inside larger NaN-filled allocations whose margins (and row gaps) must stay
NaN; in the ``strided-poisoned`` layout the INPUTS sit in NaN-filled allocations too (margins, row gaps), the checkpoints
and the workspaces start as NaN, and every output must still be finite and inside the bound.  Footprints: one non-finite
operand element may show in the outputs exactly where tests/scan_footprint.py's dependency rule says.  The tests only
detect: nothing here tries to make a kernel fault, no test makes a kernel read or write outside memory the test owns, and
non-finite VALUES are data, not addresses."""
from __future__ import annotations

import ctypes
import time

import pytest
import torch

from tests import scan_fp64_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
IO = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
WORST: dict = {}            # (kernel label, form, regime, output) -> worst err / (U S)
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
M4 = 0b1010

# (name, batch, KD, L, N, G, rev_mask, u_gshift, ckpt_pitch, IO dtype, forward family, forward in segments, backward
# family, backward in segments): launches of a few hundred rows that force each family (the sizes of FAMILIES in
# tests/test_deterministic_gpu.py), lengths that are not multiples of the tile (1283, 2564), one past a checkpoint
# (20, 164, 641, 644, 2049), N in {4, 8, 16}.  tests/test_scan_fp64_cpu.py asserts the planner's choice for each.
CASES = [
    ("rl-seg", 2, 256, 600, 16, 4, M4, 1, 16, f32, "Fwdr", True, "Bwdr", True),
    ("rl-seg-2564", 1, 256, 2564, 16, 4, M4, 1, 16, f32, "Fwdr", True, "Bwdr", True),
    ("rl-seg-4800", 1, 256, 4800, 16, 4, M4, 1, 16, f32, "Fwdr", True, "Bwdr", True),
    ("rl-one-n4", 8, 3072, 324, 4, 4, M4, 1, 16, f32, "Fwdr", False, "Bwdr", False),
    ("rl-one-n8-20", 8, 3072, 20, 8, 4, M4, 1, 16, f32, "Fwdr", False, "Bwdr", False),
    ("rl-one-fwd", 8, 2048, 600, 16, 4, M4, 1, 16, f32, "Fwdr", False, "Bwdr", True),
    ("q-seg", 2, 256, 1600, 16, 4, M4, 1, 160, f32, "Fwd", False, "Bwd4", True),
    ("q-seg-2564", 2, 256, 2564, 16, 4, M4, 1, 160, f32, "Fwd", False, "Bwd4", True),
    ("q-seg-9600", 1, 256, 9600, 16, 4, M4, 1, 160, f32, "Fwd", False, "Bwd4", True),
    ("q-seg-n4", 2, 256, 1600, 4, 4, M4, 1, 160, f32, "Fwd", False, "Bwd4", True),
    ("q-one-n8-164", 2, 256, 164, 8, 4, M4, 1, 160, f32, "Fwd", False, "Bwd4", False),
    ("q4-n8-644", 8, 1536, 644, 8, 4, M4, 1, 160, f32, "Fwd4", False, "Bwd4", False),
    ("q4-n4-324", 8, 3072, 324, 4, 4, M4, 1, 160, f32, "Fwd4", False, "Bwd4", False),
    ("q4-n16-1284", 8, 1536, 1284, 16, 4, M4, 1, 160, f32, "Fwd4", False, "Bwd4", False),
    ("b2-640-n4", 2, 256, 1600, 4, 4, M4, 1, 640, f32, "Fwd", False, "Bwd2", False),
    ("b2-640-1283", 2, 256, 1283, 16, 4, M4, 1, 640, f32, "Fwd", False, "Bwd2", False),
    ("b2-640-n8-641", 2, 256, 641, 8, 4, M4, 1, 640, f32, "Fwd", False, "Bwd2", False),
    ("b2-640-bf16", 2, 256, 1280, 16, 4, M4, 1, 640, bf16, "Fwd", False, "Bwd2", False),
    ("b2-640-f16-1283", 2, 256, 1283, 16, 4, M4, 1, 640, f16, "Fwd", False, "Bwd2", False),
    ("b2-320", 2, 256, 1600, 16, 4, M4, 1, 320, f32, "Fwd", False, "Bwd2", False),
    ("b2-320-1283", 2, 256, 1283, 16, 4, M4, 1, 320, f32, "Fwd", False, "Bwd2", False),
    ("b2-320-bf16", 2, 256, 1600, 16, 4, M4, 1, 320, bf16, "Fwd", False, "Bwd2", False),
    ("b3", 8, 3072, 320, 4, 4, M4, 1, 320, f32, "Fwd", False, "Bwd3", False),
    ("b3-324", 8, 3072, 324, 4, 4, M4, 1, 320, f32, "Fwd", False, "Bwd3", False),
    ("b3-f16", 8, 3072, 320, 4, 4, M4, 1, 320, f16, "Fwd", False, "Bwd3", False),
    ("b1", 2, 128, 3000, 16, 2, 0, 0, 0, f32, "Fwd", False, "Bwd", False),
    ("b1-n8-1283", 2, 128, 1283, 8, 2, 0, 0, 0, f32, "Fwd", False, "Bwd", False),
    ("b1-n4-2564-rev", 2, 128, 2564, 4, 2, 0b10, 0, 0, f32, "Fwd", False, "Bwd", False),
    ("b1-2049", 1, 64, 2049, 16, 2, 0, 0, 0, f32, "Fwd", False, "Bwd", False),
    ("b1-bf16", 2, 128, 3000, 16, 2, 0, 0, 0, bf16, "Fwd", False, "Bwd", False),
]
BY_NAME = {c[0]: c for c in CASES}
CORE_REGIMES = ("init", "large_dt", "threshold", "dead")         # every case
# the other regimes on one launch per kernel pair (the mid-size product is thinned here, never the regimes above)
ALL_REGIMES_ON = ("rl-seg", "rl-one-n4", "q-seg", "q4-n8-644", "b2-640-n4", "b2-320", "b3", "b1", "b2-640-bf16")
GRID = [(c[0], r) for c in CASES for r in R.REGIMES if r in CORE_REGIMES or c[0] in ALL_REGIMES_ON]


def plans(lib, batch, KD, L, N, G, mask, ush, pitch, io):
    """the planner's reports of a case's forward and backward (contiguous operands; no GPU needed)"""
    from tests.test_deterministic_cpu import bwd_params
    from sigma_amd import _capi
    bp = bwd_params(batch, KD, L, N, G, mask, ush, pitch, io)
    fp, bq = (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 6)()
    assert lib.sigma_scan_fwd_plan(ctypes.byref(bp.fwd), ctypes.byref(fp)) == 0, _capi.last_error()
    assert lib.sigma_scan_bwd_plan(ctypes.byref(bp), ctypes.byref(bq)) == 0, _capi.last_error()
    return list(fp), list(bq)


def launch_constants(shape, pitch, io=0):
    """(constants of the default form, of the deterministic form, forward family, backward family) from the planner"""
    from sigma_amd import _capi
    from tests.test_deterministic_cpu import family_of, fwd_family_of
    batch, KD, L, N, G, mask, ush = shape
    fp, bp = plans(_capi.load(), batch, KD, L, N, G, mask, ush, pitch, io)
    ff, bf = fwd_family_of(fp), family_of(bp)
    return (R.constants(ff, bf, fp, bp, batch, KD, L, N, G, det=False), R.constants(ff, bf, fp, bp, batch, KD, L, N, G, det=True), ff, bf)


def run_kernels(args, shape, pitch, io):
    """forward, default backward and deterministic backward through the binding; asserts the census keys of the case"""
    from sigma_amd import selective_scan_cuda_core as core
    from tests.test_deterministic_gpu import deterministic
    from tests.test_stream_fp64_gpu import recording, scan_case_keys
    batch, KD, L, N, G, mask, ush = shape
    u, delta, A, B, C, D, bias, dout, softplus = args
    ops = (u, delta, A, B, C, D, bias)
    kw = dict(rev_mask=mask, u_gshift=ush, ckpt_pitch=pitch)
    with recording() as launched:
        out, x = core.fwd_ext(*ops, softplus, **kw)
        grads = core.bwd_ext(*ops, dout, x, softplus, dout_gshift=ush, **kw)
        with deterministic():
            det = core.bwd_ext(*ops, dout, x, softplus, dout_gshift=ush, **kw)
    torch.cuda.synchronize()
    assert launched == scan_case_keys(batch, KD, L, N, G, mask, ush, pitch, io, det=(False, True)), launched
    return out, grads, det


def held(label, form, regime, got, ref, S, failures):
    """every output of ``got`` (name -> tensor or None) against its bound; records the worst ratio"""
    for name, t in got.items():
        if t is None:
            continue
        r = R.ratio(t, ref[name], S[name])
        key = (label, form, regime, name)
        WORST[key] = max(WORST.get(key, 0.0), r)
        print(f"  {label:22s} {form:4s} {regime:12s} {name:12s} err / (U S) = {r:.3g}")
        if not r <= 1.0:
            failures.append(f"{label} {form} {regime} {name}: {r:.3g}")


def bound_check(args, shape, pitch, io, regime, out, grads, det, failures=None):
    """the fp64 bound on the forward and both backward forms of one launch (``det`` None: the default form only);
    returns (ref, S) of the default form"""
    batch, KD, L, N, G, mask, ush = shape
    cs, cs_det, ff, bf = launch_constants(shape, pitch, io)
    from tests.test_deterministic_cpu import segments_of
    from sigma_amd import _capi
    fp, bp = plans(_capi.load(), batch, KD, L, N, G, mask, ush, pitch, io)
    tag = "" if io == 0 else "-" + {1: "float16", 2: "bfloat16"}[io]
    fl = f"{ff}{'-seg' if ff == 'Fwdr' and fp[4] > 1 else ''}-p{pitch}{tag}"
    bl = f"{bf}{'-seg' if segments_of(bp) > 1 else ''}-p{pitch}{tag}"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref, S, sums = R.reference(*args[:8], args[8], cs, rev_mask=mask, u_gshift=ush, dout_gshift=ush,
                               io={0: "float32", 1: "float16", 2: "bfloat16"}[io])
    torch.cuda.synchronize()
    print(f"  fp64 reference of {batch}x{KD}x{L}xN{N}: {time.perf_counter() - t0:.2f} s")
    own = failures if failures is not None else []
    held(fl, "fwd", regime, {"out": out}, ref, S, own)
    names = R.OUTPUTS[1:]
    held(bl, "def", regime, dict(zip(names, grads)), ref, S, own)
    if det is not None:
        held(bl, "det", regime, dict(zip(names, det)), ref, R.rebound(S, sums, cs, cs_det), own)
    if failures is None:
        assert not own, "outside the fp64 bound: " + "; ".join(own)
    return ref, S


@pytest.mark.parametrize("name,regime", GRID, ids=[f"{n}-{r}" for n, r in GRID])
def test_every_family_on_every_regime(name, regime):
    _, batch, KD, L, N, G, mask, ush, pitch, dtype, *_ = BY_NAME[name]
    args = R.make(regime, batch, KD, L, N, G, ush, seed=41, device=DEV, dtype=dtype)
    shape = (batch, KD, L, N, G, mask, ush)
    out, grads, det = run_kernels(args, shape, pitch, IO[dtype])
    bound_check(args, shape, pitch, IO[dtype], regime, out, grads, det)


# one launch per kernel pair for the negative controls
CONTROL_CASES = ("rl-seg", "rl-one-n4", "q-seg", "q4-n8-644", "b2-640-n4", "b2-320", "b3", "b1")
# (wrong fp64 variant, regime, output the kernel must fail on)
KERNEL_CONTROLS = (("bf16_decay", "init", "out"), ("exp_1e-5", "long_memory", "out"), ("drop_carry", "long_memory", "out"),
                   ("threshold10", "threshold", "out"), ("sigmoid1_10", "threshold", "ddelta"), ("adjoint_at", "init", "du"),
                   ("dA_last_image", "init", "dA"), ("dB_last_row", "init", "dB"), ("dC_last_row", "init", "dC"))


@pytest.mark.parametrize("name", CONTROL_CASES)
def test_kernel_outputs_fail_wrong_references(name):
    """sharpness, shown on the kernel's own output: against a plausible wrong fp64 variant (only reference code runs in
    it) the output named must be OUTSIDE the bound that it meets against the true reference"""
    _, batch, KD, L, N, G, mask, ush, pitch, dtype, *_ = BY_NAME[name]
    shape = (batch, KD, L, N, G, mask, ush)
    cs, _, _, _ = launch_constants(shape, pitch)
    ran = {}
    weak = []
    for wrong, regime, output in KERNEL_CONTROLS:
        if regime not in ran:
            args = R.make(regime, batch, KD, L, N, G, ush, seed=43, device=DEV, dtype=dtype)
            out, grads, _ = run_kernels(args, shape, pitch, 0)
            ran = {regime: (args, dict(zip(R.OUTPUTS, [out] + list(grads))))}         # one regime's tensors alive at a time
        args, got = ran[regime]
        # the carry dropped where a checkpoint, a tile and (row-lane, quad-row) a segment of this length begin
        bad, S, _ = R.reference(*args[:8], args[8], cs, rev_mask=mask, u_gshift=ush, dout_gshift=ush, wrong=wrong,
                                wrong_at=min(640, L // 2 // 160 * 160 or 16))
        r = R.ratio(got[output], bad[output], S[output])
        print(f"  {name:12s} {wrong:14s} {regime:12s} {output:7s} err / (U S) = {r:.3g}")
        if not r > 1.0:
            weak.append(f"{wrong} on {regime}: {output} at {r:.3g}")
    assert not weak, "the bound cannot tell the kernel from: " + "; ".join(weak)


# ---------------------------------------------------------------------------------------------------------------------
# guard bands, through the C ABI

def _guard(rows_shape, L, stride, dtype=torch.float32, margin=None):
    """(buffer, view): a rows_shape + (L,) view with row stride ``stride`` inside a NaN-filled 1-D buffer, margins of a
    row + 64 elements on both sides (multiples of 4 elements: the view keeps 16-byte alignment for f32)"""
    rows = 1
    for r in rows_shape:
        rows *= r
    m = (stride + 64 + 3) // 4 * 4
    buf = torch.full((rows * stride + 2 * m,), float("nan"), device=DEV, dtype=dtype)
    view = buf[m:m + rows * stride].view(*rows_shape, stride)[..., :L]
    return buf, view


def _intact(buf, view, what):
    assert bool(torch.isfinite(view).all()), f"{what}: interior not fully written"
    seen = view.clone()
    view.fill_(float("nan"))
    ok = bool(torch.isnan(buf).all())
    view.copy_(seen)
    assert ok, f"{what}: written outside its rows (guard band or row gap)"


def _capi_run(args, shape, pitch, pad, poison_scratch=False):
    """forward and default backward through sigma_selective_scan_fwd / _bwd directly (_bwd_capi of
    tests/test_deterministic_gpu.py, generalised): out, du, ddelta, dB, dC are views of row stride L + pad inside
    NaN-filled buffers; returns (out, grads) after checking the guard bands.  ``poison_scratch``: the checkpoints and both
    workspaces hold NaN (all bits set) before the forward instead of whatever torch.empty returns -- the flag
    torch.utils.deterministic.fill_uninitialized_memory fills nothing here, deterministic algorithms being off"""
    from sigma_amd import _capi
    from sigma_amd import selective_scan_cuda_core as core
    lib = _capi.load()
    batch, KD, L, N, G, mask, ush = shape
    u, delta, A, B, C, D, bias, dout, softplus = args
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g_out = _guard((batch, KD), L, L + pad, delta.dtype)
    g_du, g_dd = _guard((batch, KD), L, L + pad, delta.dtype), _guard((batch, KD), L, L + pad, delta.dtype)
    g_dB, g_dC = _guard((batch, G, N), L, L + pad), _guard((batch, G, N), L, L + pad)
    out, du, ddelta, dB, dC = g_out[1], g_du[1], g_dd[1], g_dB[1], g_dC[1]
    n_chunks = (L + _capi.SIGMA_SCAN_CHUNK - 1) // _capi.SIGMA_SCAN_CHUNK
    if pitch:
        x = torch.empty(batch, KD, core._ckpt_slots(L, pitch) * N, device=DEV)
    else:
        x = torch.empty(batch, KD, n_chunks, 2 * N, device=DEV)
    if poison_scratch:
        x.fill_(float("nan"))
    fp = _capi.FwdParams()
    core._fill_fwd(fp, u, delta, A, B, C, D, bias, out, x, softplus, (batch, KD, L, N, G), mask, ush, pitch, 0)
    keep = []
    if pitch == 16:
        core.rowlane_selftest(DEV)
        n = int(lib.sigma_scan_fwd_workspace_bytes(ctypes.byref(fp)))
        assert n >= 0, _capi.last_error()
        if n:
            keep.append(torch.empty(n, dtype=torch.uint8, device=DEV))
            if poison_scratch:
                keep[-1].fill_(255)
            fp.workspace, fp.workspace_bytes = keep[-1].data_ptr(), n
    _capi.check(lib.sigma_selective_scan_fwd(ctypes.byref(fp), stream), "fwd")
    dA = torch.zeros(KD, N, device=DEV)
    dD, dbias = torch.zeros(KD, device=DEV), (torch.zeros(KD, device=DEV) if bias is not None else None)
    bp = _capi.BwdParams()
    core._fill_fwd(bp.fwd, u, delta, A, B, C, D, bias, None, x, softplus, (batch, KD, L, N, G), mask, ush, pitch, 0)
    bp.dout_group_shift, bp.flags = ush, 0
    bp.dout, bp.du, bp.ddelta = dout.data_ptr(), du.data_ptr(), ddelta.data_ptr()
    bp.dA, bp.dB, bp.dC, bp.dD = dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), dD.data_ptr()
    bp.ddelta_bias = dbias.data_ptr() if dbias is not None else None
    bp.dout_batch_stride, bp.dout_d_stride = dout.stride(0), dout.stride(1)
    bp.du_batch_stride, bp.du_d_stride = du.stride(0), du.stride(1)
    bp.ddelta_batch_stride, bp.ddelta_d_stride = ddelta.stride(0), ddelta.stride(1)
    bp.dA_d_stride, bp.dA_dstate_stride = dA.stride(0), dA.stride(1)
    bp.dB_batch_stride, bp.dB_group_stride, bp.dB_dstate_stride = dB.stride()[:3]
    bp.dC_batch_stride, bp.dC_group_stride, bp.dC_dstate_stride = dC.stride()[:3]
    n = int(lib.sigma_scan_bwd_workspace_bytes(ctypes.byref(bp)))
    assert n >= 0, _capi.last_error()
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=DEV)
    if poison_scratch:
        ws.fill_(255)
    bp.workspace, bp.workspace_bytes = ws.data_ptr(), n
    _capi.check(lib.sigma_selective_scan_bwd(ctypes.byref(bp), stream), "bwd")
    torch.cuda.synchronize()
    for g, what in ((g_out, "out"), (g_du, "du"), (g_dd, "ddelta"), (g_dB, "dB"), (g_dC, "dC")):
        _intact(*g, what)
    return out, [du, ddelta, dA, dB, dC, dD, dbias]


def _strided(t, pad, offset):
    """the same values as rows of stride L + pad, starting ``offset`` elements into their allocation"""
    L = t.shape[-1]
    rows = t.numel() // L
    buf = torch.zeros(rows * (L + pad) + offset, device=t.device, dtype=t.dtype)
    v = buf[offset:].view(*t.shape[:-1], L + pad)[..., :L]
    v.copy_(t)
    return v


def _poisoned(t, pad, offset):
    """(buffer, view): the same values as rows of stride L + pad that start ``offset`` elements past a margin as large as
    _guard's, inside a NaN-filled allocation: both margins and every row gap hold NaN"""
    L = t.shape[-1]
    buf, _ = _guard(t.shape[:-1], L, L + pad, t.dtype)
    m = (buf.numel() - (t.numel() // L) * (L + pad)) // 2
    buf = torch.cat([buf, buf[:offset]])
    view = buf[m + offset:m + offset + (t.numel() // L) * (L + pad)].view(*t.shape[:-1], L + pad)[..., :L]
    view.copy_(t)
    return buf, view


GUARDED = ("rl-seg-2564", "rl-one-n8-20", "q-seg-2564", "q-one-n8-164", "q4-n8-644", "b2-640-1283", "b2-640-n8-641",
           "b2-320-1283", "b2-640-f16-1283", "b3-324", "b1-n8-1283", "b1-2049")


@pytest.mark.parametrize("layout", ["contiguous", "strided-offset", "strided-poisoned"])
@pytest.mark.parametrize("name", GUARDED)
def test_outputs_inside_nan_guard_bands(name, layout):
    """the ragged lengths, with contiguous operands and with strided operands at an offset (rows of stride L + 8 that
    start 4 elements into their allocation -- what the 16-byte kernels still take -- and outputs of stride L + 8):
    margins and row gaps stay NaN, every interior element is finite and inside the fp64 bound.  ``strided-poisoned``: the
    same strided layout with u, delta, B, C and dout inside NaN-filled allocations (margins of a row + 64 elements, row
    gaps) and the checkpoints and workspaces prefilled with NaN: a kernel that reads before a row, past its end or a
    checkpoint it never wrote, and masks the value by a product with zero, returns NaN; afterwards the gaps and margins of
    the inputs must still be NaN"""
    _, batch, KD, L, N, G, mask, ush, pitch, dtype, *_ = BY_NAME[name]
    args = list(R.make("init", batch, KD, L, N, G, ush, seed=47, device=DEV, dtype=dtype))
    pad = 0
    if layout == "strided-offset":
        pad = 8
        for i in (0, 1, 3, 4, 7):
            args[i] = _strided(args[i], pad, 4)
    bufs = {}
    if layout == "strided-poisoned":
        pad = 8
        for i in (0, 1, 3, 4, 7):
            bufs[i], args[i] = _poisoned(args[i], pad, 4)
    shape = (batch, KD, L, N, G, mask, ush)
    out, grads = _capi_run(args, shape, pitch, pad, poison_scratch=layout == "strided-poisoned")
    for i, buf in bufs.items():
        _intact(buf, args[i], f"input {'u delta A B C D bias dout'.split()[i]}")
    cs, _, _, _ = launch_constants(shape, pitch, IO[dtype])
    ref, S, _ = R.reference(*args[:8], args[8], cs, rev_mask=mask, u_gshift=ush, dout_gshift=ush,
                            io={0: "float32", 1: "float16", 2: "bfloat16"}[IO[dtype]], io_bc=False)
    bad = []
    held(f"capi {name}", layout[:4], "init", dict(zip(R.OUTPUTS, [out] + grads)), ref, S, bad)
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the footprint of one non-finite operand element (tests/scan_footprint.py)
from tests import scan_footprint as F  # noqa: E402

FOOTPRINT_CASES = CONTROL_CASES + ("rl-seg-2564", "rl-one-n8-20", "q-seg-2564", "b2-640-1283", "b1-n4-2564-rev")
PLANT_KINDS = [(op, v) for op in F.SEQ_OPERANDS for v in (F.NAN, F.INF)] + [(op, F.NAN) for op in F.ROW_OPERANDS]
FOOT_GRID = [(c, op, v) for c in FOOTPRINT_CASES for op, v in PLANT_KINDS]
TILE_OF_PITCH = {16: 16, 160: 160, 320: 320, 640: 640, 0: 2048}     # the tile dB / dC of a backward family are formed in
# Where a kernel may show a non-finite element that the rule does not: (kernel family, operand, direction of the planted
# row, output, reason, source).  Only inside the plant's own row (its own (batch, group) and tile for dB / dC); a
# non-finite element anywhere else, and a finite one inside a cone, fail whatever stands here.
_PAD = ("positions past the end of the row are walked as identity steps (dl = 0 by a select, scan_bwd.hip:189, "
        "scan_bwd2.hip:159, scan_bwd4.hip:171): a non-finite state leaving the last position is carried through them and meets "
        "dl = 0 in the dA term, 0 * NaN")
_PAD_A = ("the decay of a padded position is exp2(0 * A): NaN for a NaN A, and the adjoint enters the last position through "
          "it; du and dB of the LAST scan position only (every earlier one is in the cone anyway)")
_RCP = "u sum_n dx B is rebuilt as (dl u) (sum_n dx B / dl): inf * 0 at the plant itself, and its row's ddelta_bias sums it"
DEVIATIONS: tuple = tuple(
    [(fam, op, rev, "dA", _PAD, src) for fam, src in (("Bwd", "scan_bwd.hip:232"), ("Bwd2", "scan_bwd2.hip:214"), ("Bwd4", "scan_bwd4.hip:232"))
     for op in ("u", "B") for rev in (False, True)] +
    [(fam, "A", rev, out, _PAD_A, src) for fam, src in (("Bwd", "scan_bwd.hip:232"), ("Bwd2", "scan_bwd2.hip:214"), ("Bwd4", "scan_bwd4.hip:232"))
     for out in ("du", "dB") for rev in (False, True)] +
    [("Bwd4", "delta+inf", rev, out, _RCP, "scan_bwd4.hip:353") for out in ("ddelta", "ddelta_bias") for rev in (False, True)])
DEVIATION_HITS: dict = {}
_CLEAN: dict = {}           # the last case's unplanted problem: (args, ref, S, sums, constants) -- computed once per case


def _clean(name):
    if name not in _CLEAN:
        _CLEAN.clear()
        _, batch, KD, L, N, G, mask, ush, pitch, dtype, *_ = BY_NAME[name]
        shape = (batch, KD, L, N, G, mask, ush)
        args = R.make("init", batch, KD, L, N, G, ush, seed=59, device=DEV, dtype=dtype)
        cs, cs_det, ff, bf = launch_constants(shape, pitch, IO[dtype])
        ref, S, sums = R.reference(*args[:8], args[8], cs, rev_mask=mask, u_gshift=ush, dout_gshift=ush,
                                   io={0: "float32", 1: "float16", 2: "bfloat16"}[IO[dtype]])
        _CLEAN[name] = (args, ref, S, R.rebound(S, sums, cs, cs_det), ff, bf)
    return _CLEAN[name]


def _segment_starts(name):
    """memory positions at which a sequence segment of the case's plans begins, for a forward and for a reversed row
    (segments are runs of ceil(tiles / S) tiles in scan order)"""
    from sigma_amd import _capi
    from tests.test_deterministic_cpu import family_of, segments_of
    _, batch, KD, L, N, G, mask, ush, pitch, dtype, ff, *_ = BY_NAME[name]
    fp, bp = plans(_capi.load(), batch, KD, L, N, G, mask, ush, pitch, IO[dtype])
    out = []
    for segs, tile in ((max(fp[4], 1) if ff == "Fwdr" else 1, 16), (segments_of(bp), 160 if family_of(bp) == "Bwd4" else 16)):
        if segs > 1:
            ntiles = -(-L // tile)
            per = -(-ntiles // segs)
            out += [per * tile, (ntiles - per) * tile - 1]
    return out


@pytest.mark.parametrize("name,op,value", FOOT_GRID, ids=[f"{c}-{op}-{'nan' if v != v else 'inf'}" for c, op, v in FOOT_GRID])
def test_one_non_finite_operand_element_shows_exactly_in_its_cone(name, op, value):
    """NaN / +inf planted in single operand elements (the first four positions of a row, the last, the first of a 16-, a
    160- and a 640-tile, the first of a sequence segment; a forward and a reversed row; several plants per launch, their
    cones pairwise disjoint): in the forward, the default and the deterministic backward every element inside a cone is
    non-finite, every element outside the cones is finite and inside the fp64 bound of the UNPLANTED problem.  A kernel
    may deviate only through DEVIATIONS, only inside the plant's own row / tile."""
    _, batch, KD, L, N, G, mask, ush, pitch, dtype, *_ = BY_NAME[name]
    shape, dims = (batch, KD, L, N, G, mask, ush), (batch, KD, L, N, G)
    kw = dict(rev_mask=mask, u_gshift=ush, dout_gshift=ush)
    args, ref, S, S_det, ff, bf = _clean(name)
    ts = F.positions(L, segment_starts=_segment_starts(name))
    failures, hits = [], 0
    io = {0: "float32", 1: "float16", 2: "bfloat16"}[IO[dtype]]
    for plants in F.launches(op, value, dims, mask, ush, ush, ts):
        if op == "delta" and value == F.INF:                 # finite outside the cones, but not the unplanted values: the twin
            twin = F.plant_into(args, [F.Plant(p.operand, p.index, F.DECAYED) for p in plants])
            cs, cs_det, _, _ = launch_constants(shape, pitch, IO[dtype])
            ref, S, sums = R.reference(*twin[:8], twin[8], cs, rev_mask=mask, u_gshift=ush, dout_gshift=ush, io=io)
            S_det = R.rebound(S, sums, cs, cs_det)
        cone, own_dir = F.empty_masks(dims), {False: F.empty_masks(dims), True: F.empty_masks(dims)}
        for p in plants:                                     # cones pairwise disjoint; not vacuous: every output the operand reaches
            overlap, sizes = F.footprint(p, dims, into=cone, **kw)
            assert not overlap, (p, plants)
            assert set(sizes) & set(F.SEQ_OUTPUTS) == set(F.reached(p, dims, **kw)), (p, sizes)
            assert all(sizes[n] < cone[n].numel() for n in F.reached(p, dims, **kw)), (p, sizes)       # and a complement
            for d in (False, True):
                F.own(p, dims, TILE_OF_PITCH[pitch], only_rev=d, into=own_dir[d], **kw)
        owns = F.union([own_dir[False], own_dir[True]])
        excused = {}
        for fam, t_op, t_rev, t_out, _, _ in DEVIATIONS:
            if t_op in (op, f"{op}+inf" if value == F.INF else op) and fam == (ff if t_out == "out" else bf):
                excused[t_out] = excused[t_out] | own_dir[t_rev][t_out] if t_out in excused else own_dir[t_rev][t_out]
        out, grads, det = run_kernels(F.plant_into(args, plants), shape, pitch, IO[dtype])
        names = R.OUTPUTS[1:]
        for form, got, bound in (("fwd", {"out": out}, S), ("def", dict(zip(names, grads)), S), ("det", dict(zip(names, det)), S_det)):
            bad, devs = F.check(got, cone, owns, ref, bound, excused)
            failures += [f"{form} {[(p.index, p.value) for p in plants]} {b}" for b in bad]
            hits += sum(devs.values())
    DEVIATION_HITS[(name, op, value != value)] = hits
    print(f"  {name:16s} {op:10s} {'nan' if value != value else 'inf'}: elements excused by the deviation table: {hits}")
    assert not failures, "\n".join(failures[:12])


# ---------------------------------------------------------------------------------------------------------------------
# the dominant launch and the headline shape at full size on the regimes the existing tests never reach
FULL = [(16, 3072, 1200, 16, 4, M4, 1, 16), (16, 768, 19200, 16, 4, M4, 1, 160)]


@pytest.mark.parametrize("regime", ["large_dt", "dead", "long_memory"])
@pytest.mark.parametrize("shape", FULL, ids=["x".join(map(str, s[:3])) + f"xN{s[3]}" for s in FULL])
def test_full_size_launches_on_the_hard_regimes(shape, regime):
    batch, KD, L, N, G, mask, ush, pitch = shape
    args = R.make(regime, batch, KD, L, N, G, ush, seed=53, device=DEV)
    out, grads, det = run_kernels(args, shape[:7], pitch, 0)
    bound_check(args, shape[:7], pitch, 0, regime + " (full)", out, grads, det)


def test_zz_report_worst_ratios():
    """prints the worst err / (U S) per kernel, form, regime and output (the cases above asserted <= 1)"""
    print("\nworst |err| / (U S) per kernel (family[-seg]-pitch[-io]), form, regime: output ratio ...")
    rows: dict = {}
    for (label, form, regime, name), r in WORST.items():
        rows.setdefault((label, form, regime), {})[name] = r
    for key in sorted(rows):
        print(f"   {key[0]:24s} {key[1]:4s} {key[2]:20s} " + "  ".join(f"{n} {rows[key][n]:.3f}" for n in R.OUTPUTS if n in rows[key]))
    assert all(r <= 1.0 for r in WORST.values())
