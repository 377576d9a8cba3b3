"""Depthwise conv + SiLU through the C ABI at the smallest shapes at which a kernel of four-pixel runs, bordered LDS images
and row strips can go wrong, against the fp64 reference and error bounds of tests/test_stream_fp64_gpu.py
(test_dwconv_silu_against_fp64: the helpers are imported, not copied).

Every case runs both n_orders, both values of the deterministic bit and packed / channel-major planes.  out2, dx, gpre,
dweight, dbias and the deterministic workspace sit in NaN guard bands.  gpre is bounded with K = 24, the share that
test_dwconv_silu_against_fp64 gives "the error of gpre and the product" inside its dweight bound."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.test_stream_fp64_gpu import _dw_ref, _guarded, _intact, _rand, _stream, check, dw_plane, rejects

pytestmark = pytest.mark.gpu

# (B, d, H, W, offset): offset (floats) shifts out2 / dx / gpre off their 16-byte alignment
CASES = [
    (2, 3, 1, 1, 0), (2, 3, 1, 7, 0), (2, 3, 5, 1, 0),        # a single row, a single column, W < 4
    (1, 2, 3, 4, 0), (2, 3, 4, 6, 0),                         # W % 4 of 0 and 2
    (2, 5, 33, 37, 0),                                        # L odd: every second plane starts off a 16-byte boundary
    (2, 4, 34, 64, 0), (1, 3, 70, 130, 0),                    # more than one strip / column block: halos cross inside the plane
    (1, 2, 95, 61, 0), (1, 2, 96, 61, 0),                     # either side of the 48 KiB line of the gpre contract
    # beyond the issue's list: W % 4 == 0 with unaligned tensors (the 16-byte path must be refused on the pointers, not on
    # W alone), a two-block strip row with W % 4 == 0 (96 x 160: 96 + 64 columns), and a plane below the line that is too
    # narrow for the bordered image (compact whole-plane body)
    (2, 3, 6, 8, 1), (1, 2, 96, 160, 0), (1, 2, 1400, 1, 0),
]
_REF: dict = {}


def _reference(case):
    """x (packed values), w, b and the fp64 forward of a case: computed once, shared by its eight runs"""
    if case not in _REF:
        B, d, H, W, _ = case
        x = _rand(B, d, H, W, seed=11)
        w, b = _rand(d, 1, 3, 3, seed=12, scale=0.3), _rand(d, seed=13, scale=0.1)
        with torch.no_grad():
            pre, ab = _dw_ref(x.double(), w.double(), b.double())
            pre_r, _ = _dw_ref(x.double(), w.double(), b.double(), pad="replicate")
        _REF[case] = (x, w, b, pre, ab, pre_r)
    return _REF[case]


def _two_orders(y, orders):
    B, d, H, W = y.shape
    return torch.stack([y.reshape(B, d, H * W)] + ([y.transpose(2, 3).reshape(B, d, H * W)] if orders == 2 else []), 1)


@pytest.mark.parametrize("layout", ["packed", "cmajor"])
@pytest.mark.parametrize("orders", [2, 1], ids=["o2", "o1"])
@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}" + ("-unaligned" if c[4] else "") for c in CASES])
def test_dwconv_small_shapes_against_fp64(case, orders, layout):
    from sigma_amd import _capi
    B, d, H, W, offset = case
    L = H * W
    plane = dw_plane(H, W)
    lib = _capi.load()
    xp, w, b, pre, ab, pre_r = _reference(case)
    if layout == "cmajor":                                   # the (d, B, H, W) hand-over of in_proj: the same values
        x = xp.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
        xbs, xcs = L, B * L
    else:
        x, xbs, xcs = xp, 0, 0
    gout = _guarded((B, orders, d, L), L, offset)
    p = _capi.DwConvParams()
    p.batch, p.channels, p.height, p.width, p.n_orders = B, d, H, W, orders
    p.x, p.weight, p.bias, p.out2 = x.data_ptr(), w.data_ptr(), b.data_ptr(), gout[1].data_ptr()
    p.x_batch_stride, p.x_channel_stride = xbs, xcs
    _capi.check(lib.sigma_dwconv3x3_silu_fwd(ctypes.byref(p), _stream()), "dwconv fwd")
    torch.cuda.synchronize()
    _intact(gout, "out2")

    g2 = _rand(B, orders, d, L, seed=14)
    g64 = g2.double()
    with torch.no_grad():
        y = pre * torch.sigmoid(pre)
        S_pre = ab + b.double().abs().view(1, d, 1, 1)
        S_o = _two_orders(S_pre * (1.1 + pre.abs()), orders)
        check("dwconv shapes", gout[1], _two_orders(y, orders), S_o, 16, "out2")
        yr = pre_r * torch.sigmoid(pre_r)
        rejects(gout[1], _two_orders(yr, orders), S_o, 16, "replicate padding")
        # backward reference: gpre = (g0 + g1^T) silu'(pre), dx = conv^T(gpre, w), dweight / dbias = sums over B H W
        sg = torch.sigmoid(pre)
        gsum = g64[:, 0].view(B, d, H, W) + (g64[:, 1].view(B, d, W, H).transpose(2, 3) if orders == 2 else 0.0)
        gp_ref = gsum * sg * (1 + pre * (1 - sg))
        dx_ref = F.conv_transpose2d(gp_ref, w.double(), padding=1, groups=d)
        xpad = F.pad(xp.double(), (1, 1, 1, 1))
        dw_ref = torch.stack([(gp_ref * xpad[:, :, i:i + H, j:j + W]).sum((0, 2, 3)) for i in range(3) for j in range(3)], 1)
        db_ref = gp_ref.sum((0, 2, 3))
        ga = g64.abs()
        S_gpre = (ga[:, 0].view(B, d, H, W) + (ga[:, 1].view(B, d, W, H).transpose(2, 3) if orders == 2 else 0.0)) * (1.1 + S_pre)
        S_dx = F.conv_transpose2d(S_gpre, w.double().abs(), padding=1, groups=d)
        S_dw = torch.stack([(S_gpre * xpad.abs()[:, :, i:i + H, j:j + W]).sum((0, 2, 3)) for i in range(3) for j in range(3)], 1)
        S_db = S_gpre.sum((0, 2, 3))
    tiles = 1 if plane else -(-H // 32) * -(-W // 32)
    depth = (-(-L // 256) if plane else 4) + 6 + 3                       # the serial depth of one workgroup's sums
    results = {}
    for det in (False, True):
        p.flags = _capi.SIGMA_DWCONV_DETERMINISTIC if det else 0
        nws = int(lib.sigma_dwconv3x3_silu_bwd_workspace_bytes(ctypes.byref(p)))
        assert nws == (B * tiles * d * 40 if det else 0)
        gws = _guarded((max(nws // 4, 4),), 64)
        gdx = _guarded((B, d, H, W) if layout == "packed" else (d, B, H, W), L, offset if layout == "packed" else 0)
        dxv = gdx[1] if layout == "packed" else gdx[1].permute(1, 0, 2, 3)
        ggp = _guarded((B, d, H, W), L, offset)
        gdw, gdb = _guarded((d, 9), 64), _guarded((d,), 64)
        if not det:                                          # the default mode accumulates, the deterministic one writes
            gdw[1].zero_()
            gdb[1].zero_()
        p.g2, p.gpre, p.dweight, p.dbias, p.dx = g2.data_ptr(), ggp[1].data_ptr(), gdw[1].data_ptr(), gdb[1].data_ptr(), gdx[1].data_ptr()
        p.workspace, p.workspace_bytes = (gws[1].data_ptr(), nws) if det else (None, 0)
        _capi.check(lib.sigma_dwconv3x3_silu_bwd(ctypes.byref(p), _stream()), f"dwconv bwd (det={det})")
        torch.cuda.synchronize()
        for g_, what in ((gws, "workspace"), (gdx, "dx"), (ggp, "gpre"), (gdw, "dweight"), (gdb, "dbias")):
            _intact(g_, f"{what} (det={det})")
        if not det:
            assert bool(torch.isnan(gws[1]).all()), "workspace written without the deterministic bit"
        K = depth + 24 + B * tiles
        with torch.no_grad():
            check("dwconv shapes", dxv, dx_ref, S_dx, 33, f"dx (det={det})")
            if plane:                                        # below the 48 KiB line gpre stays on chip
                assert bool(torch.isnan(ggp[1]).all()), "gpre touched below the 48 KiB line"
            else:
                check("dwconv shapes", ggp[1], gp_ref, S_gpre, 24, f"gpre (det={det})")
            check("dwconv shapes", gdw[1], dw_ref, S_dw, K, f"dweight (det={det})")
            check("dwconv shapes", gdb[1], db_ref, S_db, K, f"dbias (det={det})")
            if B > 1:
                rejects(gdb[1], gp_ref[:-1].sum((0, 2, 3)), S_db, K, f"dbias missing the last image (det={det})")
        results[det] = (dxv.clone(), ggp[1].clone(), gdw[1].clone(), gdb[1].clone())
        if det:                                              # bitwise repeatable: a second call over fresh NaN
            gdw[1].fill_(float("nan"))
            gdb[1].fill_(float("nan"))
            _capi.check(lib.sigma_dwconv3x3_silu_bwd(ctypes.byref(p), _stream()), "dwconv bwd (deterministic, again)")
            torch.cuda.synchronize()
            assert torch.equal(gdw[1], results[True][2]) and torch.equal(gdb[1], results[True][3]), "deterministic sums differ between two calls"
    assert torch.equal(results[True][0], results[False][0]), "dx: deterministic mode changed it"
    if not plane:
        assert torch.equal(results[True][1], results[False][1]), "gpre: deterministic mode changed it"
