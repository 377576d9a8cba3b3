"""The stream kernels through the C ABI at their edge shapes (Part A) and on value regimes (Part B); run with -m gpu.

Shapes, regimes, fp64 twins and the derivations of the three additions to S are in tests/stream_regimes.py; K and S are
those of the matching test of tests/test_stream_fp64_gpu.py, whose helpers are imported, not copied.  Every output sits in
a NaN guard band.  A test id is a kernel times a family: the shapes of a family are walked inside the test, and the
failing shape is named in the assertion.  tests/test_stream_regimes_cpu.py holds the fp32 emulation under the same bounds
and the wrong variants rejected, so nothing here passes vacuously.

Non-finite containment: the oracle is the twin's own finiteness (``_contained``).  Wherever the twin is finite the kernel
must be finite and inside the unchanged bound; wherever it is not, the kernel must not be either (inf against NaN is not
told apart)."""
import ctypes
import time

import pytest
import torch

from tests import stream_regimes as sr
from tests.test_dwconv_shapes_gpu import _two_orders
from tests.test_stream_fp64_gpu import (WORST, _dw_ref, _guarded, _intact, _rand, _stream, _up_ref, check, ln_nv, record,  # noqa: F401
                                        rejects)

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRE = "regimes: "
_SPENT = [0.0]


@pytest.fixture(autouse=True)
def _clock():
    """adds up the time spent inside this file's tests (setup of their fixtures excluded)"""
    t0 = time.time()
    yield
    _SPENT[0] += time.time() - t0


def _c(t):
    return ctypes.c_void_p(t.data_ptr())


def _d(t):
    return None if t is None else t.double()


def _contained(family, got, ref, S, K, what):
    r, share, ok = sr.contained(got, ref, S, K)
    assert ok, f"{what}: the kernel and the twin are not finite in the same places"
    WORST[PRE + family] = max(WORST.get(PRE + family, 0.0), r)
    assert r <= 1.0, f"{what}: max |err| / (K u S) = {r:.3g} over the finite part (K = {K})"
    return share


def _bits(a, b):
    """equal, with NaN equal to NaN"""
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan], b[~nan])


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm

def _ln_run(x, gamma, beta, *, z=None, zs=0, rsc=None, rps=0, dy=None, dadd=None, stats=True, dbeta=True, dzs=0,
            inplace=False):
    """sigma_layernorm_fwd (+ _bwd when dy is given) with every output in a guard band.  z: the gate VIEW (rows, C) with
    row stride zs; dzs: dgate_row_stride (0 = contiguous), the gradient is the last C columns of a (rows, dzs) buffer;
    inplace: dx_add is dx itself, prefilled with dadd.  Returns (outputs, guards, partial rows)."""
    from sigma_amd import _capi
    lib = _capi.load()
    rows, C = x.shape
    g = dict(y=_guarded((rows, C), C))
    p = _capi.LayerNormParams()
    p.rows, p.channels, p.eps = rows, C, sr.EPS
    p.x, p.gamma, p.y = x.data_ptr(), gamma.data_ptr(), g["y"][1].data_ptr()
    p.beta = beta.data_ptr() if beta is not None else None
    if stats:
        g["mean"], g["rstd"] = _guarded((rows,), 1), _guarded((rows,), 1)
        p.mean, p.rstd = g["mean"][1].data_ptr(), g["rstd"][1].data_ptr()
    if z is not None:
        assert z.stride(0) == zs and z.stride(1) == 1 and z.data_ptr() % 16 == 0
        p.gate, p.gate_row_stride = z.data_ptr(), zs
    if rsc is not None:
        p.row_scale, p.rows_per_scale = rsc.data_ptr(), rps
    _capi.check(lib.sigma_layernorm_fwd(ctypes.byref(p), _stream()), "layernorm_fwd")
    nw = int(lib.sigma_layernorm_bwd_partial_rows(rows, C))
    out = {k: v[1] for k, v in g.items()}
    if dy is not None:
        assert stats
        ws = torch.full((max(nw, 1) * 2 * C,), float("nan"), device=DEV)
        g["dx"], g["dgamma"] = _guarded((rows, C), C), _guarded((C,), C)
        p.dy, p.dx, p.dgamma, p.workspace = dy.data_ptr(), g["dx"][1].data_ptr(), g["dgamma"][1].data_ptr(), ws.data_ptr()
        if dbeta:
            g["dbeta"] = _guarded((C,), C)
            p.dbeta = g["dbeta"][1].data_ptr()
        if inplace:
            g["dx"][1].copy_(dadd)
            p.dx_add = g["dx"][1].data_ptr()
        elif dadd is not None:
            p.dx_add = dadd.data_ptr()
        if z is not None:
            width = dzs if dzs else C
            g["dzbuf"] = _guarded((rows, width), width)
            dzv = g["dzbuf"][1][:, width - C:]
            p.dgate, p.dgate_row_stride = dzv.data_ptr(), dzs
        _capi.check(lib.sigma_layernorm_bwd(ctypes.byref(p), _stream()), "layernorm_bwd")
        out = {k: v[1] for k, v in g.items()}
        if z is not None:
            out["dz"] = dzv
    torch.cuda.synchronize()
    for k, v in g.items():
        _intact(v, k)
    if z is not None and dy is not None and dzs > C:
        assert bool(torch.isnan(g["dzbuf"][1][:, :dzs - C]).all()), "dz: the columns in front of the gate half were written"
    return out, nw


_LN_OUT = (("y", "S_y"), ("mean", "S_mean"), ("rstd", "S_rstd"), ("dx", "S_dx"), ("dgamma", "S_dg"), ("dbeta", "S_db"), ("dz", "S_dz"))


def _ln_compare(family, out, t, K, what, contain=False):
    for name, S in _LN_OUT:
        if name in out and name in t:
            if contain:
                _contained(family, out[name], t[name], t[S], K[name], f"{what} {name}")
            else:
                check(PRE + family, out[name], t[name], t[S], K[name], f"{what} {name}")


def _gate_buffer(zval, zs):
    """the gate values (rows, C) as the LAST C columns of a (rows, zs) buffer whose other columns are NaN"""
    rows, C = zval.shape
    zz = torch.full((rows, zs), float("nan"), device=DEV)
    zz[:, zs - C:] = zval
    return zz[:, zs - C:]


def _ln_inputs(rows, C, variant, nsamp=None, seed=0):
    """the inputs of test_layernorm_against_fp64 (x = 0.3 + 0.02 randn: eps is 2.5 % of the variance; dy correlated with
    xhat), the row factors of ``sr.factors`` when the variant has them"""
    gated, scaled, dxa = variant.startswith("gated"), variant == "gated_rs", variant == "dx_add"
    x = _rand(rows, C, seed=seed + 1, scale=0.02, mean=0.3)
    gamma, beta = _rand(C, seed=seed + 2, scale=0.5, mean=1.0), _rand(C, seed=seed + 3, scale=0.1)
    z = _gate_buffer(_rand(rows, C, seed=seed + 4), 2 * C) if gated else None
    dy = 25.0 * (x - x.mean(1, keepdim=True)) + _rand(rows, C, seed=seed + 5)
    dadd = _rand(rows, C, seed=seed + 6) if dxa else None
    rsc = rps = rs_rows = None
    if scaled:
        nsamp = nsamp or rows
        rps = rows // nsamp
        assert rps * nsamp == rows
        rsc = torch.tensor(sr.factors(nsamp), device=DEV)
        rs_rows = rsc.repeat_interleave(rps)
    return dict(x=x, gamma=gamma, beta=beta, z=z, dy=dy, dadd=dadd, rsc=rsc, rps=rps, rs_rows=rs_rows)


def _ln_case(rows, C, variant, record, nsamp=None, family="layernorm shapes"):
    """one shape of Part A: launch keys, guard bands, every output under the unchanged bound, the negative controls of
    test_layernorm_against_fp64 that make sense at the shape; returns (inputs, outputs, twin, K, partial rows)"""
    gated, scaled, dxa = variant.startswith("gated"), variant == "gated_rs", variant == "dx_add"
    what = f"{rows}x{C} {variant}"
    i = _ln_inputs(rows, C, variant, nsamp)
    del record[:]
    out, nw = _ln_run(i["x"], i["gamma"], i["beta"], z=i["z"], zs=2 * C, rsc=i["rsc"], rps=i["rps"] or 0, dy=i["dy"], dadd=i["dadd"],
                      dzs=2 * C if gated else 0)
    assert record == [("ln_fwd", ln_nv(C), gated, scaled), ("ln_bwd", ln_nv(C), gated, scaled, dxa)], (what, record)
    K = sr.ln_K(rows, C, nw)
    args = (_d(i["x"]), _d(i["gamma"]), _d(i["beta"]), sr.EPS, K, _d(i["z"]), _d(i["rs_rows"]), _d(i["dy"]), _d(i["dadd"]))
    t = sr.ln_twin(*args)
    _ln_compare(family, out, t, K, what)
    live = (i["rs_rows"] != 0) if scaled else torch.ones(rows, dtype=torch.bool, device=DEV)
    if bool(live.any()):
        rejects(out["y"][live], sr.ln_twin(*args[:7], eps_out=True)["y"][live], t["S_y"][live], K["y"], f"{what}: eps outside the sqrt")
        if C >= 256:
            rejects(out["y"][live], sr.ln_twin(*args[:7], unbiased=True)["y"][live], t["S_y"][live], K["y"], f"{what}: unbiased variance")
    if scaled:                                             # a dropped sample: exact zeros (x is finite)
        dead = ~live
        for name in ("y", "dz", "dx"):
            assert bool((out[name][dead] == 0).all()), f"{what}: {name} of a zero-factor sample is not exactly 0"
    return i, out, t, K, nw


@pytest.mark.parametrize("variant", sr.LN_VARIANTS)
def test_layernorm_with_fewer_rows_than_waves(variant, record):
    """rows in {1, 2, 3, 4, 5, 7} x C in {4, 8, 252, 256, 260}: idle waves, one live lane (C = 4), the NV = 1 / 2 edge; the
    gated_rs variant has one sample per row"""
    for rows, C in sr.LN_SMALL:
        _ln_case(rows, C, variant, record)


@pytest.mark.parametrize("case", sr.LN_WALK, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_layernorm_walks_several_rows_per_wave(case, record):
    """20001 rows: every wave walks two or three rows and the last step of most waves leaves the prefetch chain (NV <= 2).
    Negative control: dgamma without the rows of the last walk step."""
    from sigma_amd import _capi
    rows, C, variant = case
    nw = int(_capi.load().sigma_layernorm_bwd_partial_rows(rows, C))
    assert rows > 4 * nw and rows > 8192
    i, out, t, K, nw = _ln_case(rows, C, variant, record, nsamp=1, family="layernorm walk")
    tail = rows % (4 * nw) or 4 * nw
    s = torch.sigmoid(_d(i["z"])) * _d(i["z"]) if i["z"] is not None else 1.0
    gpre = _d(i["dy"]) * s * (_d(i["rs_rows"])[:, None] if i["rs_rows"] is not None else 1.0)
    rejects(out["dgamma"], (gpre * t["xh"])[:rows - tail].sum(0), t["S_dg"], K["dgamma"], "dgamma missing the last row block")


@pytest.mark.parametrize("case", sr.LN_FACTOR, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_layernorm_row_factor_carry(case, record):
    """the per-wave carry of the stochastic-depth factor over 3 to 16 samples: several steps of the carry loop per walk step
    (1200 and 4001 rows per sample), one row per wave (3 x 7) and one sample per row.  Negative control: the factors
    shifted by one sample."""
    nsamp, rps, C = case
    rows = nsamp * rps
    i, out, t, K, nw = _ln_case(rows, C, "gated_rs", record, nsamp=nsamp, family="layernorm row factor")
    if rps >= 1200:                                        # the point of the case: a walk step crosses more than one sample
        assert 4 * nw > rps, f"{4 * nw} waves do not step over a sample of {rps} rows"
    shifted = torch.roll(i["rsc"], 1).repeat_interleave(rps)
    w = sr.ln_twin(_d(i["x"]), _d(i["gamma"]), _d(i["beta"]), sr.EPS, K, _d(i["z"]), _d(shifted), _d(i["dy"]))
    for name, S in (("y", "S_y"), ("dx", "S_dx"), ("dz", "S_dz")):
        # the bound of the RIGHT factors, plus the wrong ones' own magnitude where the right factor is 0 (S = 0 there)
        rejects(out[name], w[name], t[S] + w[S], K[name], f"{name} with the factors shifted by one sample")


@pytest.mark.parametrize("case", [(7, 260), (300, 96), (2100, 772)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_layernorm_optional_operands(case, record):
    """beta == NULL (plain and gated, dbeta == NULL with it), the forward without mean / rstd, dx_add == dx, gate row
    strides C, 2C and 2C + 4, dgate_row_stride 0 and 2C"""
    rows, C = case
    fam = "layernorm options"
    # beta == NULL
    for variant in ("plain", "gated"):
        i = _ln_inputs(rows, C, variant, seed=10)
        out, nw = _ln_run(i["x"], i["gamma"], None, z=i["z"], zs=2 * C, dy=i["dy"], dbeta=False, dzs=2 * C if i["z"] is not None else 0)
        K = sr.ln_K(rows, C, nw)
        t = sr.ln_twin(_d(i["x"]), _d(i["gamma"]), None, sr.EPS, K, _d(i["z"]), None, _d(i["dy"]))
        assert "dbeta" not in out
        _ln_compare(fam, out, t, K, f"{rows}x{C} {variant} without beta")
        wb = sr.ln_twin(_d(i["x"]), _d(i["gamma"]), _d(i["beta"]), sr.EPS, K, _d(i["z"]), None, _d(i["dy"]))
        rejects(out["y"], wb["y"], t["S_y"] + wb["S_y"], K["y"], "y with a beta that was not given")
        if variant == "gated":
            rejects(out["dz"], wb["dz"], t["S_dz"] + wb["S_dz"], K["dz"], "dz with a beta that was not given")
    # forward without the statistics: the same bits
    i = _ln_inputs(rows, C, "gated_rs", nsamp=1, seed=20)
    full, _ = _ln_run(i["x"], i["gamma"], i["beta"], z=i["z"], zs=2 * C, rsc=i["rsc"], rps=rows)
    bare, _ = _ln_run(i["x"], i["gamma"], i["beta"], z=i["z"], zs=2 * C, rsc=i["rsc"], rps=rows, stats=False)
    assert "mean" not in bare and torch.equal(full["y"], bare["y"]), "the forward without mean / rstd gives other bits"
    # dx_add == dx: the same bits as a separate addend
    i = _ln_inputs(rows, C, "dx_add", seed=30)
    sep, nw = _ln_run(i["x"], i["gamma"], i["beta"], dy=i["dy"], dadd=i["dadd"])
    inp, _ = _ln_run(i["x"], i["gamma"], i["beta"], dy=i["dy"], dadd=i["dadd"], inplace=True)
    K = sr.ln_K(rows, C, nw)
    t = sr.ln_twin(_d(i["x"]), _d(i["gamma"]), _d(i["beta"]), sr.EPS, K, None, None, _d(i["dy"]), _d(i["dadd"]))
    _ln_compare(fam, inp, t, K, f"{rows}x{C} dx_add in place")
    assert torch.equal(sep["dx"], inp["dx"]), "dx_add == dx gives other bits than a separate addend"
    rejects(inp["dx"], t["dx"] - _d(i["dadd"]), t["S_dx"], K["dx"], "dx without its addend")
    # gate and dgate strides
    i = _ln_inputs(rows, C, "gated", seed=40)
    zval = i["z"].contiguous()
    first = None
    for zs in (C, 2 * C, 2 * C + 4):
        for dzs in (0, 2 * C):
            out, nw = _ln_run(i["x"], i["gamma"], i["beta"], z=_gate_buffer(zval, zs), zs=zs, dy=i["dy"], dzs=dzs)
            K = sr.ln_K(rows, C, nw)
            if first is None:
                t = sr.ln_twin(_d(i["x"]), _d(i["gamma"]), _d(i["beta"]), sr.EPS, K, _d(zval), None, _d(i["dy"]))
                _ln_compare(fam, out, t, K, f"{rows}x{C} gate stride {zs}")
                first = out
            for name in ("y", "dx", "dz", "dgamma", "dbeta"):
                assert torch.equal(out[name], first[name]), f"{name}: gate stride {zs} / dgate stride {dzs} changes the bits"
    zrot = torch.roll(zval, 1, 0)
    rejects(first["y"], sr.ln_twin(_d(i["x"]), _d(i["gamma"]), _d(i["beta"]), sr.EPS, K, _d(zrot))["y"], t["S_y"], K["y"], "the gate of the row above")


# ---------------------------------------------------------------------------------------------------------------------
# cross merge / split, transpose2d, pair_sum_add, bilinear x2

def _merge_run(p4, nh):
    from sigma_amd import _capi
    B, _, d, L = p4.shape
    _, H, W, _ = nh.shape
    gm, gs = _guarded((B, H, W, d), d), _guarded((B, 2, d, L), L)
    p = _capi.MergeParams()
    p.batch, p.channels, p.height, p.width = B, d, H, W
    p.planes4, p.nhwc = p4.data_ptr(), gm[1].data_ptr()
    _capi.check(_capi.load().sigma_cross_merge_nhwc(ctypes.byref(p), _stream()), "merge")
    p.planes2, p.nhwc = gs[1].data_ptr(), nh.data_ptr()
    _capi.check(_capi.load().sigma_cross_split_nhwc(ctypes.byref(p), _stream()), "split")
    torch.cuda.synchronize()
    _intact(gm, "merge")
    _intact(gs, "split")
    return gm[1], gs[1]


_merge_ref = sr.merge_ref


def test_cross_merge_split_edge_shapes(record):
    """extents of 1, channel counts around the 32-channel tile, grids of every residue mod 8 (sr.MERGE_CASES).  Merge: K = 3;
    split: a copy, exact.  Negative control: the memory orders swapped, where the two orders differ (H != W, both > 1)."""
    controls = 0
    for B, d, H, W in sr.MERGE_CASES:
        what = f"{B}x{d}x{H}x{W} (grid {sr.merge_grid(B, d, H, W)})"
        p4, nh = _rand(B, 4, d, H * W, seed=21), _rand(B, H, W, d, seed=22)
        del record[:]
        m, s = _merge_run(p4, nh)
        assert record == [("merge",), ("split",)]
        ref, S, want = _merge_ref(p4, nh)
        check(PRE + "merge shapes", m, ref, S, 3, f"merge {what}")
        assert torch.equal(s, want), f"split {what}"
        if H != W and min(H, W) > 1:
            rejects(m, _merge_ref(p4, nh, swapped=True)[0], S, 3, f"merge with swapped orders {what}")
            assert not torch.equal(s, want.flip(1))
            controls += 1
    assert controls >= 20


def _transpose_run(src, R, C, drs):
    from sigma_amd import _capi
    B, _, srs = src.shape
    g = _guarded((B, C, drs), drs)
    p = _capi.TransposeParams()
    p.batch, p.rows, p.cols = B, R, C
    p.src, p.dst = src.data_ptr(), g[1].data_ptr()
    p.src_batch_stride, p.src_row_stride, p.dst_batch_stride, p.dst_row_stride = R * srs, srs, C * drs, drs
    _capi.check(_capi.load().sigma_transpose2d(ctypes.byref(p), _stream()), "transpose2d")
    torch.cuda.synchronize()
    _intact(g, "transpose")
    return g[1]


def test_transpose2d_edge_shapes(record):
    """rows and cols in {1, 31, 32, 33}, row strides equal to the extent and larger and odd, batch 1 and 3: exact, the
    padding of the destination rows untouched.  Negative control: the untransposed copy."""
    for B, R, C, pad in sr.TR_CASES:
        srs, drs = C + pad, R + (pad + 2 if pad else 0)
        src = _rand(B, R, srs, seed=31)
        dst = _transpose_run(src, R, C, drs)
        what = f"{B}x{R}x{C} strides {srs}, {drs}"
        assert torch.equal(dst[:, :, :R], src[:, :, :C].transpose(1, 2)), what
        assert bool(torch.isnan(dst[:, :, R:]).all()), f"{what}: wrote the padding of the destination rows"
        if R != C and min(R, C) > 1:
            assert not torch.equal(dst[:, :, :R].reshape(-1), src[:, :, :C].reshape(-1))
    assert record == [("transpose",)] * len(sr.TR_CASES)


def _pair_sum_run(src, acc0, off):
    from sigma_amd import _capi
    no, inner = acc0.shape
    ga = _guarded((no, inner), inner, offset=off)
    ga[1].copy_(acc0)
    _capi.check(_capi.load().sigma_pair_sum_add(_c(src), _c(ga[1]), no, inner, _stream()), "pair_sum_add")
    torch.cuda.synchronize()
    _intact(ga, "pair_sum_add")
    return ga[1]


def test_pair_sum_add_edge_shapes(record):
    """inner of 1, 3, 4, 5, 4096, 4100 with one and two outer indices, and 65535, 65536, 70001 outer indices (the gridDim.y cap)
    at inner = 4; 16-byte aligned and 4-byte offset views.  K = 3.  Negative control: only one of the pair added."""
    for no, inner, off in sr.PS_CASES:
        src = _rand(2 * no * inner + off, seed=41)[off:].view(no, 2, inner)
        acc0 = _rand(no, inner, seed=42)
        del record[:]
        got = _pair_sum_run(src, acc0, off)
        what = f"{no}x{inner} offset {off}"
        assert record == [("pair_sum_add", "vec" if inner % 4 == 0 and not off else "scalar")], (what, record)
        s = src.double()
        S = acc0.double().abs() + s.abs().sum(1)
        check(PRE + "pair_sum shapes", got, acc0.double() + s.sum(1), S, 3, what)
        rejects(got, acc0.double() + s[:, 0], S, 3, f"one of the pair {what}")
        if no > 65535:                                      # the rows past the cap, on their own
            rejects(got[65535:], acc0.double()[65535:], S[65535:], 3, f"rows past gridDim.y untouched {what}")


def _upsample_run(x, g):
    from sigma_amd import _capi
    B, H, W, C = x.shape
    lib = _capi.load()
    go, gi = _guarded((B, 2 * H, 2 * W, C), 2 * W * C), _guarded((B, H, W, C), W * C)
    _capi.check(lib.sigma_upsample2x_nhwc(_c(x), _c(go[1]), B, H, W, C, 0, _stream()), "up")
    _capi.check(lib.sigma_upsample2x_nhwc(_c(g), _c(gi[1]), B, H, W, C, 1, _stream()), "up adj")
    torch.cuda.synchronize()
    _intact(go, "upsample")
    _intact(gi, "upsample adjoint")
    return go[1], gi[1]


def test_upsample2x_edge_shapes(record):
    """extents of 1 and 2 in either direction (every output a border output).  Forward K = 6 on sum |w x|, adjoint K = 18
    on the adjoint of |g|.  Negative control: align_corners=True, where it differs."""
    controls = 0
    for B, H, W, C in sr.UP_CASES:
        x, g = _rand(B, H, W, C, seed=51), _rand(B, 2 * H, 2 * W, C, seed=52)
        del record[:]
        out, din = _upsample_run(x, g)
        assert record == [("upsample", "fwd"), ("upsample", "adjoint")]
        what = f"{B}x{H}x{W}x{C}"
        S = _up_ref(x.double().abs())
        check(PRE + "upsample shapes", out, _up_ref(x.double()), S, 6, f"forward {what}")
        check(PRE + "upsample shapes", din, sr.up_adjoint(g.double()), sr.up_adjoint(g.double().abs()), 18, f"adjoint {what}")
        wrong = _up_ref(x.double(), align_corners=True)
        if not torch.equal(wrong, _up_ref(x.double())):
            rejects(out, wrong, S, 6, f"align_corners=True {what}")
            controls += 1
    assert controls >= 5


# ---------------------------------------------------------------------------------------------------------------------
# ChannelAttention plane ops, colscale_bwd

def _offset_copy(t, off):
    """t in a fresh buffer, ``off`` floats past its 16-byte alignment"""
    buf = torch.empty(t.numel() + off, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def _plane_run(x, g, s, dm, dmx, off):
    from sigma_amd import _capi
    lib = _capi.load()
    P, hw = x.shape
    o = dict(mean=_guarded((P,), 1, offset=off), max=_guarded((P,), 1), count=_guarded((P,), 1), scale=_guarded((P, hw), hw, offset=off),
             dot=_guarded((P,), 1), gate_bwd=_guarded((P, hw), hw, offset=off))
    _capi.check(lib.sigma_plane_pool(_c(x), P, hw, _c(o["mean"][1]), _c(o["max"][1]), _c(o["count"][1]), _stream()), "pool")
    _capi.check(lib.sigma_plane_scale(_c(x), _c(s), _c(o["scale"][1]), P, hw, _stream()), "scale")
    _capi.check(lib.sigma_plane_dot(_c(g), _c(x), _c(o["dot"][1]), P, hw, _stream()), "dot")
    q = _capi.GateBwdParams()
    q.planes, q.hw = P, hw
    q.g, q.x, q.scale, q.dmean, q.dmax = g.data_ptr(), x.data_ptr(), s.data_ptr(), dm.data_ptr(), dmx.data_ptr()
    q.max, q.count, q.dx = o["max"][1].data_ptr(), o["count"][1].data_ptr(), o["gate_bwd"][1].data_ptr()
    _capi.check(lib.sigma_plane_gate_bwd(ctypes.byref(q), _stream()), "gate_bwd")
    torch.cuda.synchronize()
    for k, v in o.items():
        _intact(v, k)
    return {k: v[1] for k, v in o.items()}


_plane_twin = sr.plane_twin
_PLANE_K = lambda hw: dict(mean=-(-hw // 256) + 10, dot=-(-hw // 256) + 10, scale=2, gate_bwd=5)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("P", [1, 3])
def test_plane_ops_edge_shapes(P, off, record):
    """hw of 1 to 5, around one wave (63 - 65), around one pass of the workgroup (255 - 257) and of its float4s (1023 - 1025).
    Planes: two maxima in different waves, a constant plane (count == hw), the maximum in the last element (of the scalar
    tail where there is one).  Max and count exact.  Negative controls: mean / dot without the last element of each plane."""
    for hw in sr.PLANE_HW:
        x = _offset_copy(sr.plane_inputs(P, hw, ("tied", "constant", "last"), seed=61 + hw, device=DEV), off)
        g = _offset_copy(_rand(P, hw, seed=63), off)
        s, dm, dmx = _rand(P, seed=62), _rand(P, seed=64), _rand(P, seed=65)
        del record[:]
        o = _plane_run(x, g, s, dm, dmx, off)
        v = "vec" if hw % 4 == 0 and not off else "scalar"
        what = f"{P}x{hw} offset {off}"
        assert record == [("plane_pool", v), ("plane_scale", v), ("plane_dot", v), ("plane_gate_bwd", v)], (what, record)
        t, K = _plane_twin(x, g, s, dm, dmx), _PLANE_K(hw)
        assert torch.equal(o["max"].double(), t["max"]) and torch.equal(o["count"].double(), t["count"]), f"max / count {what}"
        assert t["count"].tolist() == [min(2, hw), hw, 1][:P]
        for name in ("mean", "scale", "dot", "gate_bwd"):
            check(PRE + "plane shapes", o[name], t[name], t["S_" + name], K[name], f"{name} {what}")
        if hw > 1:
            xd, gd = x.double(), g.double()
            rejects(o["mean"], xd[:, :-1].sum(1) / hw, t["S_mean"], K["mean"], f"mean without the last element {what}")
            rejects(o["dot"], (gd * xd)[:, :-1].sum(1), t["S_dot"], K["dot"], f"dot without the last element {what}")


@pytest.mark.parametrize("hw", [5, 64, 257, 1000, 1001, 1024])
def test_plane_ops_with_infinite_planes(hw, record):
    """planted ties of Part A that are not finite: a plane of all -inf (max -inf, count hw) and a plane whose maximum is
    +inf twice, next to an ordinary tied plane.  Max and count exact; the other outputs non-finite exactly where the twin
    is and inside the bounds elsewhere."""
    x = sr.plane_inputs(3, hw, ("neg_inf", "pos_inf", "tied"), seed=66, device=DEV)
    g = _rand(3, hw, seed=63)
    s, dm, dmx = _rand(3, seed=62), _rand(3, seed=64), _rand(3, seed=65)
    o = _plane_run(x, g, s, dm, dmx, 0)
    t, K = _plane_twin(x, g, s, dm, dmx), _PLANE_K(hw)
    what = f"3x{hw}"
    assert torch.equal(o["max"].double(), t["max"]) and torch.equal(o["count"].double(), t["count"]), f"max / count {what}"
    assert t["count"].tolist() == [hw, 2, 2]
    for name in ("mean", "scale", "dot", "gate_bwd"):
        _contained("plane infinite", o[name], t[name], t["S_" + name], K[name], f"{name} {what}")
    assert float(o["mean"][0]) == -sr.INF and float(o["mean"][1]) == sr.INF
    assert bool(torch.isfinite(o["gate_bwd"][0]).all()), "gate_bwd of an all -inf plane: every element is a maximum"


@pytest.mark.parametrize("value", sr.POISONS, ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("hw", [1000, 1001])
def test_plane_ops_contain_non_finite_values(hw, value, record):
    """24 planes, one pixel of plane 5 of x and one pixel of plane 17 of g poisoned (``sr.plane_poison_inputs``): the other
    22 planes of every output inside the bounds, max and count as torch.amax and == give them (a NaN is the maximum of its
    plane, count 0), the two planes non-finite exactly where the twin is.  Negative control: the twin of the planes
    without the poison."""
    x, g, s, dm, dmx = sr.plane_poison_inputs(hw, value, 66, DEV)
    o = _plane_run(x, g, s, dm, dmx, 0)
    t, K = _plane_twin(x, g, s, dm, dmx), _PLANE_K(hw)
    what = f"24x{hw} {value}"
    assert _bits(o["max"], t["max"].float()), f"max {what}: {o['max'].tolist()} against {t['max'].tolist()}"
    assert torch.equal(o["count"].double(), t["count"]), f"count {what}"
    assert float(t["count"][5]) == (0 if value != value else 1 if value > 0 else 2)
    for name in ("mean", "scale", "dot", "gate_bwd"):
        assert _contained("plane non-finite", o[name], t[name], t["S_" + name], K[name], f"{name} {what}") >= 0.9
    xc, gc = x.clone(), g.clone()
    xc[5, hw // 2], gc[17, hw - 1] = 0.0, 0.0
    clean = _plane_twin(xc, gc, s, dm, dmx)
    for name in ("mean", "dot"):
        assert not sr.contained(o[name], clean[name], clean["S_" + name], K[name])[2], f"{name}: the unpoisoned twin is not told apart"


def _colscale_run(dy, x, s, ws_form):
    from sigma_amd import _capi
    lib = _capi.load()
    rows, C = x.shape
    gdx, gds = _guarded((rows, C), C), _guarded((C,), C)
    if not ws_form:
        gds[1].zero_()
        _capi.check(lib.sigma_colscale_bwd(_c(dy), _c(x), _c(s), _c(gdx[1]), _c(gds[1]), rows, C, _stream()), "colscale_bwd")
        gws = None
    else:
        n = int(lib.sigma_colscale_bwd_workspace_bytes(rows, C))
        gws = _guarded((n // 4,), C)
        _capi.check(lib.sigma_colscale_bwd_ws(_c(dy), _c(x), _c(s), _c(gdx[1]), _c(gds[1]), rows, C, _c(gws[1]), n, _stream()), "colscale_bwd_ws")
    torch.cuda.synchronize()
    for g_, w_ in ((gdx, "dx"), (gds, "ds")) + (((gws, "workspace"),) if gws else ()):
        _intact(g_, w_)
    return gdx[1], gds[1]


def _colscale_K(rows, C):
    slots = 256 // (C // 4)
    G = min(512, -(-rows // slots))
    deep = -(-rows // (G * slots))
    return slots, G, deep + slots + G + 2, deep + slots + -(-G // 16) + 16 + 2


@pytest.mark.parametrize("C", sr.CS_C)
def test_colscale_bwd_edge_shapes(C, record):
    """rows of 1, slots - 1, slots, slots + 1 and 512 slots + 1 (one row in a second grid-stride step), chunk counts that
    leave idle threads (C = 96: 16, C = 516: 127), both entry points; the deterministic form twice over fresh NaN: the
    same bits.  Negative control: ds without the last row (the whole last grid-stride block at 512 slots + 1 rows, where
    the row is made 32 times larger so that one row in 512 slots shows under a K of slots + 512)."""
    for rows in sr.cs_rows(C):
        slots, G, Ka, Kd = _colscale_K(rows, C)
        x = _rand(rows, C, seed=71).abs()
        dy = 0.5 * x + _rand(rows, C, seed=72)
        if rows > G * slots:
            assert rows - G * slots == 1
            x[-1] *= 32.0
            dy[-1] *= 32.0
        s = _rand(C, seed=73)
        dd, xd = dy.double(), x.double()
        S = (dd * xd).abs().sum(0)
        what = f"{rows}x{C}"
        del record[:]
        dx, ds = _colscale_run(dy, x, s, False)
        dx1, ds1 = _colscale_run(dy, x, s, True)
        dx2, ds2 = _colscale_run(dy, x, s, True)
        assert record == [("colscale_bwd", slots)] + [("colscale_bwd_ws", slots)] * 2, (what, record)
        check(PRE + "colscale shapes", dx, dd * s.double(), (dd * s.double()).abs(), 2, f"dx {what}")
        assert torch.equal(dx, dx1) and torch.equal(dx1, dx2) and torch.equal(ds1, ds2), f"{what}: the deterministic form is not repeatable"
        check(PRE + "colscale shapes", ds, (dd * xd).sum(0), S, Ka, f"ds {what}")
        check(PRE + "colscale shapes", ds1, (dd * xd).sum(0), S, Kd, f"ds (deterministic) {what}")
        rejects(ds, (dd * xd)[:-1].sum(0), S, Ka, f"ds missing the last row {what}")
        rejects(ds1, (dd * xd)[:-1].sum(0), S, Kd, f"deterministic ds missing the last row {what}")


# ---------------------------------------------------------------------------------------------------------------------
# Part B: value regimes

def _three_samples(rs, rows):
    """(row_scale, rows_per_scale) of the per-row factors of ``sr.ln_case``: three samples of rows / 3 rows"""
    if rs is None:
        return None, 0
    rsc = torch.tensor(sr.factors(3), device=DEV)
    assert rows % 3 == 0 and torch.equal(rsc.repeat_interleave(rows // 3), rs)
    return rsc, rows // 3


def _regime_case(rows, C, variant, regime, gate="normal", seed=900):
    """the inputs of ``sr.ln_case`` (what the CPU test runs the emulation on), on the device, the gate in the second half of
    a (rows, 2C) buffer"""
    x, gamma, beta, z, rs, dy, dadd = sr.ln_case(rows, C, variant, regime, seed, gate)
    dev = lambda t: None if t is None else t.to(DEV)
    return dev(x), dev(gamma), dev(beta), (_gate_buffer(z.to(DEV), 2 * C) if z is not None else None), dev(rs), dev(dy), dev(dadd)


@pytest.mark.parametrize("case", sr.LN_REGIME_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("regime", sr.LN_REGIMES)
def test_layernorm_value_regimes(regime, case, record):
    """all four variants on offset / constant / wide / outlier rows under the unchanged bounds (rstd with the second-order
    term of the mean's error, tests/stream_regimes.py).  Negative controls: the one-pass variance on ``offset``, eps outside
    the square root on ``constant`` and on the small end of ``wide``, a missing outlier on ``outlier``."""
    rows, C = case
    for variant in sr.LN_VARIANTS:
        x, gamma, beta, z, rs, dy, dadd = _regime_case(rows, C, variant, regime)
        rsc, rps = _three_samples(rs, rows)
        out, nw = _ln_run(x, gamma, beta, z=z, zs=2 * C, rsc=rsc, rps=rps, dy=dy, dadd=dadd,
                          dzs=2 * C if z is not None else 0)
        K = sr.ln_K(rows, C, nw)
        args = (_d(x), _d(gamma), _d(beta), sr.EPS, K, _d(z), _d(rs), _d(dy), _d(dadd))
        t = sr.ln_twin(*args, second_order=True)
        _ln_compare(f"layernorm {regime}", out, t, K, f"{rows}x{C} {variant} {regime}")
        if variant != "plain":
            continue
        if regime == "offset":
            bad = sr.ln_emulate(x, gamma, beta, sr.EPS, onepass=True)["y"]
            fin = torch.isfinite(bad).all(1)
            assert bool(fin.any())
            rejects(out["y"][fin], bad[fin].double(), t["S_y"][fin], K["y"], "one-pass variance")
        elif regime in ("constant", "wide"):
            small = slice(0, 30 if regime == "wide" else rows)
            w = sr.ln_twin(*args[:5], eps_out=True)
            rejects(out["rstd"][small], w["rstd"][small], t["S_rstd"][small], K["rstd"], f"eps outside the sqrt ({regime})")
        else:
            xo = x.clone()
            xo[xo == 1e4] = 0.0
            rejects(out["y"], sr.ln_twin(_d(xo), *args[1:5])["y"], t["S_y"], K["y"], "the row without its outlier")


@pytest.mark.parametrize("case", sr.LN_REGIME_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("variant", ["gated", "gated_rs"])
def test_layernorm_saturated_gates(variant, case, record):
    """gates of +-20 ... +-200: y, dz, dx, dgamma, dbeta under the bounds with the argument-error and underflow terms in S.
    Negative controls: the gate clamped at +-60 (also on the negative gates alone); silu' without its z (1 - sigma) term;
    sigma flushed to zero below -15, on the negative saturated gates and on those of -20 alone."""
    rows, C = case
    x, gamma, beta, z, rs, dy, dadd = _regime_case(rows, C, variant, "base", gate="saturated")
    rsc, rps = _three_samples(rs, rows)
    out, nw = _ln_run(x, gamma, beta, z=z, zs=2 * C, rsc=rsc, rps=rps, dy=dy, dzs=2 * C)
    K = sr.ln_K(rows, C, nw)
    t = sr.ln_twin(_d(x), _d(gamma), _d(beta), sr.EPS, K, _d(z), _d(rs), _d(dy), saturated=True)
    _ln_compare("layernorm saturated", out, t, K, f"{rows}x{C} {variant} saturated")
    w = sr.ln_twin(_d(x), _d(gamma), _d(beta), sr.EPS, K, _d(z).clamp(-60, 60), _d(rs), _d(dy))
    rejects(out["y"], w["y"], t["S_y"], K["y"], "gate clamped at +-60")
    a = _d(dy) * (_d(rs)[:, None] if rs is not None else 1.0)
    rejects(out["dz"], a * t["n"] * torch.sigmoid(_d(z)), t["S_dz"], K["dz"], "silu' without its z (1 - sigma) term")
    # the negative side, on the saturated negative gates alone (rows of a zero factor apart: they are exact zeros)
    live = (rs != 0)[:, None] if rs is not None else torch.ones(rows, 1, dtype=torch.bool, device=DEV)
    for sel, where in (((z <= -20.0) & live, "below -15"), ((z == -20.0) & live, "at z = -20")):
        for name, S in (("y", "S_y"), ("dz", "S_dz")):
            rejects(out[name][sel], sr.flushed(_d(z), t[name])[sel], t[S][sel], K[name], f"{name}: sigma flushed to zero {where}")
    far = (z <= -88.0) & live
    rejects(out["y"][far], w["y"][far], t["S_y"][far], K["y"], "gate clamped at -60, negative gates alone")


@pytest.mark.parametrize("case", [(300, 260), (9003, 96), (300, 1024)], ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("variant,target", [("plain", "x"), ("plain", "dy"), ("gated_rs", "x"), ("gated_rs", "gate"), ("gated_rs", "dy")])
def test_layernorm_contains_non_finite_values(variant, target, case, record):
    """NaN, +inf, -inf in turn in one element of the first row, the last row and the last row wave 0 walks under every grid
    the host can choose (x), or of one of the latter alone (gate, dy): every other row's y, dx, dz, mean and rstd inside the bound, dbeta finite and inside its
    bound under a poisoned x, the poisoned rows non-finite exactly where the twin is"""
    from sigma_amd import _capi
    rows, C = case
    x, gamma, beta, z, rs, dy, dadd = _regime_case(rows, C, variant, "base")
    rsc = rps = None
    if rs is not None:                                    # no dropped sample here: 0 * NaN is tested by the twin, not asked of the kernel
        rsc, rps = torch.tensor([1.0 / 0.9, 1.0, 2.0], device=DEV), rows // 3
        rs = rsc.repeat_interleave(rps)
    prow = sr.ln_poison_rows(rows)                         # for every grid the forward or the backward can have
    one = prow[len(prow) // 2]
    assert sr.ln_last_row_of_wave0(rows, 4 * int(_capi.load().sigma_layernorm_bwd_partial_rows(rows, C))) in prow
    for v in sr.POISONS:
        xx, dd = x.clone(), dy.clone()
        zz = _gate_buffer(z.contiguous(), 2 * C) if z is not None else None
        if target == "x":
            xx[prow, 5] = v
        else:
            (zz if target == "gate" else dd)[one, 5] = v
        out, nw = _ln_run(xx, gamma, beta, z=zz, zs=2 * C, rsc=rsc, rps=rps or 0, dy=dd, dzs=2 * C if zz is not None else 0)
        K = sr.ln_K(rows, C, nw)
        t = sr.ln_twin(_d(xx), _d(gamma), _d(beta), sr.EPS, K, _d(zz), _d(rs), _d(dd))
        _ln_compare("layernorm non-finite", out, t, K, f"{rows}x{C} {variant} {target}={v}", contain=True)
        if target == "x":
            assert bool(torch.isfinite(out["dbeta"]).all()), "dbeta does not read x"
        # negative control: the twin of the unpoisoned inputs is finite where the kernel's output is not
        clean = sr.ln_twin(_d(x), _d(gamma), _d(beta), sr.EPS, K, _d(z), _d(rs), _d(dy))
        assert not sr.contained(out["dx"], clean["dx"], clean["S_dx"], K["dx"])[2], "the unpoisoned twin is not told apart"


@pytest.mark.parametrize("value", sr.POISONS, ids=["nan", "+inf", "-inf"])
def test_layout_kernels_contain_non_finite_values(value, record):
    """merge / split / transpose / pair_sum_add / upsample with one poisoned pixel (a border and an interior one for the
    upsample): the outputs that read it are non-finite, every other output is inside its bound (copies: bit for bit)"""
    (B, d, H, W), e4, en = sr.MERGE_POISON
    p4, nh = _rand(B, 4, d, H * W, seed=21), _rand(B, H, W, d, seed=22)
    p4[e4], nh[en] = value, value
    m, s = _merge_run(p4, nh)
    ref, S, want = _merge_ref(p4, nh)
    assert int((~torch.isfinite(ref)).sum()) == 1
    _contained("layout non-finite", m, ref, S, 3, "merge")
    assert _bits(s, want), "split"
    src = _rand(3, 33, 38, seed=31)
    src[1, 32, 31] = value
    dst = _transpose_run(src, 33, 33, 40)
    assert _bits(dst[:, :, :33], src[:, :, :33].transpose(1, 2)), "transpose"
    for no, inner, off in sr.PAIR_POISON:
        src0, acc0 = sr.pair_poison_inputs(no, inner, value, 41, DEV)
        srcp = torch.empty(2 * no * inner + off, device=DEV)[off:].view(no, 2, inner)
        srcp.copy_(src0)
        got = _pair_sum_run(srcp, acc0, off)
        sd = srcp.double()
        share = _contained("layout non-finite", got, acc0.double() + sd.sum(1), acc0.double().abs() + sd.abs().sum(1), 3, "pair_sum_add")
        assert share >= 0.9
    B, H, W, C = 2, 9, 11, 4
    for y, x_ in ((0, 0), (H - 1, W - 1), (4, 5), (0, 1)):
        x, g = _rand(B, H, W, C, seed=51), _rand(B, 2 * H, 2 * W, C, seed=52)
        x[1, y, x_, 2] = value
        g[1, 2 * y, 2 * x_, 2] = value
        out, din = _upsample_run(x, g)
        f64, a64 = _up_ref(x.double()), sr.up_adjoint(g.double())
        fwd, adj = sr.up_readers(H, W, y, x_)[0], sr.up_readers(H, W, 2 * y, 2 * x_)[1]
        assert int((~torch.isfinite(f64)).sum()) == len(fwd) and int((~torch.isfinite(a64)).sum()) == len(adj)
        S = torch.nan_to_num(_up_ref(x.double().abs()), nan=sr.INF)
        Sa = torch.nan_to_num(sr.up_adjoint(g.double().abs()), nan=sr.INF)
        assert _contained("layout non-finite", out, f64, torch.where(torch.isfinite(f64), S, torch.zeros_like(S)), 6, f"upsample ({y}, {x_})") >= 0.9
        assert _contained("layout non-finite", din, a64, torch.where(torch.isfinite(a64), Sa, torch.zeros_like(Sa)), 18, f"adjoint ({y}, {x_})") >= 0.9


@pytest.mark.parametrize("value", sr.POISONS, ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("C", [96, 516])
def test_colscale_contains_non_finite_values(C, value, record):
    """one poisoned dy element (its dx element and its ds column) and one poisoned x element (its ds column alone)"""
    rows = sr.CS_POISON_ROWS
    slots, G, Ka, Kd = _colscale_K(rows, C)
    dy, x, s = sr.colscale_poison_inputs(C, value, 71, DEV)
    dd, xd = dy.double(), x.double()
    for ws_form, K in ((False, Ka), (True, Kd)):
        dx, ds = _colscale_run(dy, x, s, ws_form)
        _contained("colscale non-finite", dx, dd * s.double(), (dd * s.double()).abs(), 2, "dx")
        ref = (dd * xd).sum(0)
        assert int((~torch.isfinite(ref)).sum()) == 2
        assert _contained("colscale non-finite", ds, ref, (dd * xd).abs().sum(0), K, "ds") >= 0.9
        clean = torch.nan_to_num(dd, 0.0, 0.0, 0.0) * torch.nan_to_num(xd, 0.0, 0.0, 0.0)       # negative control
        assert not sr.contained(ds, clean.sum(0), clean.abs().sum(0), K)[2], "ds of the inputs without the poison is not told apart"


@pytest.mark.parametrize("case", [(300, 96), (300, 516), (129, 1024)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_colscale_and_plane_dot_keep_their_relative_bound_under_scales(case, record):
    """per-column (colscale) and per-plane (dot, mean, scale) factors 2^e, e from -40 to 40, on x and their inverse pattern
    on dy: the relative bounds hold unchanged, no output is flushed or overflows"""
    rows, C = case
    slots, G, Ka, Kd = _colscale_K(rows, C)
    cx, cy = sr.scales_pow2(C, 5).to(DEV), sr.scales_pow2(C, 6).to(DEV)
    x = (_rand(rows, C, seed=71).abs() + 0.01) * cx
    dy = (0.5 * _rand(rows, C, seed=74).abs() + _rand(rows, C, seed=72)) * cy
    s = _rand(C, seed=73) * sr.scales_pow2(C, 7).to(DEV)
    dd, xd = dy.double(), x.double()
    for ws_form, K in ((False, Ka), (True, Kd)):
        dx, ds = _colscale_run(dy, x, s, ws_form)
        check(PRE + "colscale scales", dx, dd * s.double(), (dd * s.double()).abs(), 2, "dx")
        check(PRE + "colscale scales", ds, (dd * xd).sum(0), (dd * xd).abs().sum(0), K, "ds")
        rejects(ds, (dd * xd)[:-1].sum(0), (dd * xd).abs().sum(0), K, "ds missing the last row")
    for P, hw in ((6, 1000), (6, 1001)):
        px = sr.scales_pow2(P, 8).to(DEV)[:, None]
        xp = sr.plane_inputs(P, hw, ("tied", "constant", "last"), seed=61, device=DEV) * px
        g = _rand(P, hw, seed=63) * sr.scales_pow2(P, 9).to(DEV)[:, None]
        sc, dm, dmx = _rand(P, seed=62), _rand(P, seed=64) * px[:, 0], _rand(P, seed=65) * px[:, 0]
        o = _plane_run(xp, g, sc, dm, dmx, 0)
        t, K = _plane_twin(xp, g, sc, dm, dmx), _PLANE_K(hw)
        assert torch.equal(o["max"].double(), t["max"]) and torch.equal(o["count"].double(), t["count"])
        for name in ("mean", "scale", "dot", "gate_bwd"):
            check(PRE + "plane scales", o[name], t[name], t["S_" + name], K[name], f"{name} {P}x{hw}")
        rejects(o["dot"], (g.double() * xp.double())[:, :-1].sum(1), t["S_dot"], K["dot"], "dot without the last element")


# ---------------------------------------------------------------------------------------------------------------------
# depthwise conv + SiLU

def _dw_run(x, w, b, g2, orders, layout, det, record):
    """sigma_dwconv3x3_silu_fwd and _bwd with every output (and the deterministic workspace) in a guard band; x is the
    packed (B, d, H, W) tensor, handed over channel-major for layout "cmajor".  Returns the outputs, dx as (B, d, H, W)."""
    from sigma_amd import _capi
    from tests.test_stream_fp64_gpu import dw_plane
    lib = _capi.load()
    B, d, H, W = x.shape
    L = H * W
    if layout == "cmajor":
        xs = x.permute(1, 0, 2, 3).contiguous()
        xbs, xcs = L, B * L
    else:
        xs, xbs, xcs = x.contiguous(), 0, 0
    g = dict(out2=_guarded((B, orders, d, L), L))
    p = _capi.DwConvParams()
    p.batch, p.channels, p.height, p.width, p.n_orders = B, d, H, W, orders
    p.x, p.weight, p.bias, p.out2 = xs.data_ptr(), w.data_ptr(), b.data_ptr(), g["out2"][1].data_ptr()
    p.x_batch_stride, p.x_channel_stride = xbs, xcs
    del record[:]
    _capi.check(lib.sigma_dwconv3x3_silu_fwd(ctypes.byref(p), _stream()), "dwconv fwd")
    p.flags = _capi.SIGMA_DWCONV_DETERMINISTIC if det else 0
    nws = int(lib.sigma_dwconv3x3_silu_bwd_workspace_bytes(ctypes.byref(p)))
    g["workspace"] = _guarded((max(nws // 4, 4),), 64)
    g["dx"] = _guarded((B, d, H, W) if layout == "packed" else (d, B, H, W), L)
    g["gpre"], g["dweight"], g["dbias"] = _guarded((B, d, H, W), L), _guarded((d, 9), 64), _guarded((d,), 64)
    if not det:
        g["dweight"][1].zero_()
        g["dbias"][1].zero_()
    p.g2, p.gpre, p.dweight, p.dbias, p.dx = g2.data_ptr(), g["gpre"][1].data_ptr(), g["dweight"][1].data_ptr(), g["dbias"][1].data_ptr(), g["dx"][1].data_ptr()
    p.workspace, p.workspace_bytes = (g["workspace"][1].data_ptr(), nws) if det else (None, 0)
    _capi.check(lib.sigma_dwconv3x3_silu_bwd(ctypes.byref(p), _stream()), "dwconv bwd")
    torch.cuda.synchronize()
    path, strided = "plane" if dw_plane(H, W) else "tiled", layout == "cmajor"
    assert record == [("dw_fwd", path, orders, strided), ("dw_bwd", path, orders, strided, det)], record
    assert path == {(6, 8): "plane", (34, 64): "plane", (96, 61): "tiled"}[(H, W)]      # what the three shapes are there for
    for k, v in g.items():
        _intact(v, k)
    out = {k: v[1] for k, v in g.items()}
    if layout == "cmajor":
        out["dx"] = out["dx"].permute(1, 0, 2, 3)
    if dw_plane(H, W):                                      # below the 48 KiB line gpre stays on chip
        assert bool(torch.isnan(out.pop("gpre")).all()), "gpre touched below the 48 KiB line"
    return out, dw_plane(H, W)


_DW_OUT = ("out2", "gpre", "dx", "dweight", "dbias")


@pytest.mark.parametrize("layout", ["packed", "cmajor"])
@pytest.mark.parametrize("case", sr.DW_CASES, ids=str)
def test_dwconv_saturated_pre_activations(case, layout, record):
    """pre-activations of +-20 ... +-200 (``sr.dw_saturated_inputs``), both n_orders and both values of the deterministic
    bit: out2, gpre, dx, dweight, dbias under the bounds with the argument-error and underflow terms in S.  Negative
    controls: the pre-activation clamped at +-60; dbias without the last image."""
    B, d, H, W = case
    for rnd in range(sr.dw_rounds(case)):
        for orders in (2, 1):
            x, w, b, g2, v = (t.to(DEV) for t in sr.dw_saturated_inputs(case, rnd, 910, orders))
            for det in (False, True):
                out, plane = _dw_run(x, w, b, g2, orders, layout, det, record)
                K = sr.dw_K(case, plane)
                t = sr.dw_twin(_d(x), _d(w), _d(b), _d(g2), orders, K, saturated=True)
                what = f"{case} {layout} o{orders} det={det} round {rnd}"
                for name in _DW_OUT:
                    if name in out:
                        check(PRE + "dwconv saturated", out[name], t[name], t["S_" + name], K[name], f"{name} {what}")
                if float(v.abs().max()) > 60:
                    wrong = sr.dw_twin(_d(x), _d(w), _d(b), _d(g2), orders, K, clamp=60.0)
                    rejects(out["out2"], wrong["out2"], t["S_out2"], K["out2"], f"pre clamped at +-60 {what}")
                if B > 1:
                    rejects(out["dbias"], t["gpre"][:-1].sum((0, 2, 3)), t["S_dbias"], K["dbias"], f"dbias missing the last image {what}")


@pytest.mark.parametrize("value", sr.POISONS, ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("case", sr.DW_CASES, ids=str)
def test_dwconv_contains_non_finite_values(case, value, record):
    """one poisoned input pixel (a corner, a border and an interior one in turn) or one poisoned element of either half of
    g2: out2 changes in exactly the 3 x 3 neighbourhood, in both memory orders, dx in the 5 x 5 one (3 x 3 for g2), the
    sums in the pixel's channel alone; everything else inside the unchanged bounds.  Packed and channel-major planes, both
    values of the deterministic bit."""
    B, d, H, W = case
    x0, w, b, g0 = (t.to(DEV) for t in sr.dw_inputs(case, 920))
    spots = ((0, 0), (H - 1, W // 2), (H // 2, W // 2))
    runs = [("x", s) for s in spots] + [("g2 row-major", spots[2]), ("g2 column-major", spots[1])]
    for n, (target, (h, w_)) in enumerate(runs):
        x, g2 = x0.clone(), g0.clone()
        if target == "x":
            x[B - 1, 1, h, w_] = value
        elif target == "g2 row-major":
            g2[B - 1, 0, 1, h * W + w_] = value
        else:
            g2[B - 1, 1, 1, w_ * H + h] = value
        layout, det = ("packed", "cmajor")[n % 2], bool(n // 2 % 2)
        out, plane = _dw_run(x, w, b, g2, 2, layout, det, record)
        K = sr.dw_K(case, plane)
        t = sr.dw_twin(_d(x), _d(w), _d(b), _d(g2), 2, K)
        near = len(sr.dw_neighbours(H, W, h, w_))
        assert int((~torch.isfinite(t["out2"])).sum()) == (2 * near if target == "x" else 0)
        assert int((~torch.isfinite(t["dx"])).sum()) == len(sr.dw_neighbours(H, W, h, w_, 2 if target == "x" else 1))
        for name in _DW_OUT:
            if name in out:
                share = _contained("dwconv non-finite", out[name], t[name], t["S_" + name], K[name], f"{name} {case} {target} ({h}, {w_}) {layout} det={det}")
                assert share >= (0.9 if name in ("out2", "gpre", "dx") else 1.0 - 1.0 / d - 1e-9)
        clean = sr.dw_twin(_d(x0), _d(w), _d(b), _d(g0), 2, K)        # negative control: the twin without the poison
        assert not sr.contained(out["dx"], clean["dx"], clean["S_dx"], K["dx"])[2], "the unpoisoned twin is not told apart"


@pytest.mark.parametrize("case", sr.DW_CASES, ids=str)
def test_dwconv_keeps_its_bounds_under_wide_inputs(case, record):
    """inputs scaled per plane by 2^e, e from -40 to 30, upstream gradients by 2^e, e from -40 to 40 (the weights stay of
    order one, so the pre-activations run from 1e-12 to 1e9 and saturate on both sides): the bounds with the saturation terms hold.
    Negative control: replicate padding (seen at the planes of small scale: S grows with the square of the pre-activation)."""
    B, d, H, W = case
    x, w, b, g2 = (t.to(DEV) for t in sr.dw_inputs(case, 930))
    e = torch.tensor([(0, 30, -40, 12, -20, 24, -8, 6)[i % 8] for i in range(B * d)], device=DEV)
    x = x * (2.0 ** e).view(B, d, 1, 1)                      # the first plane keeps its scale: the control is seen there
    g2 = g2 * sr.scales_pow2(B * d, 12).to(DEV).view(B, 1, d, 1)
    for layout, det in (("packed", False), ("cmajor", True)):
        out, plane = _dw_run(x, w, b, g2, 2, layout, det, record)
        K = sr.dw_K(case, plane)
        t = sr.dw_twin(_d(x), _d(w), _d(b), _d(g2), 2, K, saturated=True)
        for name in _DW_OUT:
            if name in out:
                check(PRE + "dwconv wide", out[name], t[name], t["S_" + name], K[name], f"{name} {case} {layout} det={det}")
        pre_r = _dw_ref(_d(x), _d(w), _d(b), pad="replicate")[0]
        rejects(out["out2"], _two_orders(pre_r * torch.sigmoid(pre_r), 2), t["S_out2"], K["out2"], "replicate padding")


def test_zz_report_worst_ratios():
    """prints the worst error / bound ratio per kernel family and regime (the cases above asserted <= 1) and the time spent
    inside this file's tests"""
    print("\nworst |err| / (K u S) per kernel and regime:")
    for fam, r in sorted(WORST.items()):
        if fam.startswith(PRE):
            print(f"   {fam[len(PRE):]:28s} {r:.3g}")
    print(f"time spent in the tests of tests/test_stream_regimes_gpu.py: {_SPENT[0]:.1f} s")
