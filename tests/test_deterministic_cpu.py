"""Deterministic mode on the host side (no GPU): the ABI 11 fields, the workspace queries with and without the
deterministic bits, and the gfx950 ISA of the deterministic kernel instantiations (no float atomics; the row-lane one keeps
its hand-counted wait)."""
import concurrent.futures as cf
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from sigma_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (batch, KD, L, N, G, rev_mask, u_gshift, ckpt_pitch, io_dtype, family, workspace bytes WITHOUT the flag: the answers of
# the tree before deterministic mode existed -- the flag-clear contract must not move.  The two row-lane answers are
# those less the hand-over area of the chained walk, (row blocks * (N * 64 + 1)) floats = 3148800 and 49200 bytes, which
# left the workspace with the walk in ABI 13: 12 dB + dC slab pairs; 3 slab pairs + the summaries of 40 segments)
SHAPES = [
    (16, 3072, 1200, 16, 4, 0b1010, 1, 16, 0, "Bwdr", 117964800),
    (1, 768, 19200, 16, 4, 0b1010, 1, 16, 0, "Bwdr", 33325056),        # row-lane with sequence segments
    (16, 768, 19200, 16, 4, 0b1010, 1, 160, 0, "Bwd4", 629145600),
    (1, 768, 19200, 16, 4, 0b1010, 1, 160, 0, "Bwd4", 79331328),        # quad-row with sequence segments
    (8, 768, 19200, 4, 4, 0b1010, 1, 640, 0, "Bwd2", 157286400),
    (8, 768, 19200, 4, 4, 0b1010, 1, 640, 2, "Bwd2", 157286400),        # bf16 IO
    (16, 6144, 300, 16, 4, 0b1010, 1, 320, 0, "Bwd2", 9830400),
    (8, 3072, 1200, 4, 4, 0b1010, 1, 320, 0, "Bwd3", 9830400),
    (2, 128, 3000, 16, 2, 0, 0, 0, 0, "Bwd", 12288000),
]


def bwd_params(B, KD, L, N, G, mask, ush, pitch, io, flags=0):
    """query parameters of a (B, KD, L) problem with contiguous operands, D and delta_bias (pointers are not read)"""
    bp = _capi.BwdParams()
    f = bp.fwd
    f.batch, f.dim, f.seqlen, f.dstate, f.n_groups = B, KD, L, N, G
    f.n_chunks = (L + 2047) // 2048
    f.io_dtype, f.delta_softplus = io, 1
    f.rev_group_mask, f.u_group_shift, f.ckpt_pitch = mask, ush, pitch
    if pitch:
        f.x_row_stride = ((L + pitch - 1) // pitch) * N
    f.u_batch_stride, f.u_d_stride = (KD >> ush) * L, L
    f.delta_batch_stride, f.delta_d_stride = KD * L, L
    f.A_d_stride, f.A_dstate_stride = N, 1
    for t in ("B", "C"):
        setattr(f, t + "_batch_stride", G * N * L); setattr(f, t + "_group_stride", N * L); setattr(f, t + "_dstate_stride", L)
    f.out_batch_stride, f.out_d_stride = KD * L, L
    f.D, f.delta_bias = 16, 16                  # non-NULL: dD / ddelta_bias are part of the problem
    bp.dout_group_shift = ush
    bp.dout_batch_stride, bp.dout_d_stride = (KD >> ush) * L, L
    bp.du_batch_stride, bp.du_d_stride = KD * L, L
    bp.ddelta_batch_stride, bp.ddelta_d_stride = KD * L, L
    bp.dA_d_stride, bp.dA_dstate_stride = N, 1
    for t in ("dB", "dC"):
        setattr(bp, t + "_batch_stride", G * N * L); setattr(bp, t + "_group_stride", N * L); setattr(bp, t + "_dstate_stride", L)
    bp.flags = flags
    return bp


def family_of(plan):
    """the backward family a plan report describes (include/sigma_scan.h, sigma_scan_bwd_plan)"""
    if plan[5] == -200:
        return "Bwdr"
    if plan[5] <= -100:
        return "Bwd4"
    if plan[4] < 0 and plan[5] < 0:
        return "Bwd3"
    if plan[4] < 0:
        return "Bwd2"
    return "Bwd"


def fwd_family_of(plan):
    """the forward family a plan report describes (sigma_scan_fwd_plan: states_per_block slot -200 row-lane, -100 quad-row)"""
    return {-200: "Fwdr", -100: "Fwd4"}.get(plan[5], "Fwd")


def segments_of(plan):
    """sequence segments of a backward plan report: quad-row items = 10 + 1000 S, row-lane tiles slot = S, else one"""
    family = family_of(plan)
    if family == "Bwd4":
        return max(plan[0] // 1000, 1)
    return max(plan[4], 1) if family == "Bwdr" else 1


def row_sum_depth(plan, batch, L):
    """Summation depth K of the per-row sums dD = sum dout u and ddelta_bias = sum ddelta over (batch, L), for the two
    forms of the backward: (K default, K deterministic).  Per family, from the kernel:
    * Bwdr (scan_bwdr.hip): four lanes per row, each adds 4 positions of every 16-tile of its segment serially
      (seg_tiles = ceil(ceil(L / 16) / S) tiles), 2 DPP levels, one result per workgroup;
    * Bwd4 (scan_bwd4.hip): 16 lanes per row, 10 positions each per 160-tile, 4 levels (row_sum_to_lane0), one result per
      tile of the segment;
    * Bwd2 (scan_bwd2.hip): 64 lanes, T = items positions each per 64 T tile, 6 levels (wave_sum), one result per tile.
    Default: every result is an atomicAdd into the zero-filled row, batch x S x (results per workgroup) of them.
    Deterministic: the results of a workgroup are added into its slot (read-add-write), then reduce_partials_det_kernel adds
    the rpart_K = batch x S slots in order."""
    family, S = family_of(plan), segments_of(plan)
    if family == "Bwdr":
        seg_tiles = -(-(-(-L // 16)) // S)
        lane, levels, per_wg = 4 * seg_tiles, 2, 1
    elif family == "Bwd4":
        seg_tiles = -(-(-(-L // 160)) // S)
        lane, levels, per_wg = 10, 4, seg_tiles
    elif family == "Bwd2":
        lane, levels, per_wg = plan[0], 6, -(-L // (64 * plan[0]))
    else:
        raise ValueError(f"no row-sum depth written out for {family}")
    return lane + levels + batch * S * per_wg, lane + levels + per_wg + batch * S


def test_abi_version_13_and_struct_fields(tmp_path):
    lib = _capi.load()
    assert _capi.SIGMA_SCAN_ABI_VERSION == 13 and lib.sigma_scan_abi_version() == 13
    fields = [("sigma_scan_bwd_params", "flags", _capi.BwdParams), ("sigma_dwconv_params", "flags", _capi.DwConvParams),
              ("sigma_dwconv_params", "workspace", _capi.DwConvParams),
              ("sigma_dwconv_params", "workspace_bytes", _capi.DwConvParams)]
    src = tmp_path / "fields.c"
    body = "".join(f'printf("%zu %zu\\n", offsetof({c}, {f}), sizeof({c}));' for c, f, _ in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigma_scan.h"\n#include "sigma_ops.h"\n'
                   'int main(void){' + body + 'printf("%d %d\\n", SIGMA_SCAN_BWD_DETERMINISTIC, '
                   'SIGMA_DWCONV_DETERMINISTIC); return 0;}')
    exe = tmp_path / "fields"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    for (c, f, cls), line in zip(fields, out):
        off, size = map(int, line.split())
        assert getattr(cls, f).offset == off and ctypes.sizeof(cls) == size, (c, f)
    assert out[len(fields)].split() == [str(_capi.SIGMA_SCAN_BWD_DETERMINISTIC), str(_capi.SIGMA_DWCONV_DETERMINISTIC)]
    # the dwconv struct grew at its end only
    assert _capi.DwConvParams.x_channel_stride.offset + 8 == _capi.DwConvParams.workspace.offset


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[9]}-{s[0]}x{s[1]}x{s[2]}xN{s[3]}-io{s[8]}" for s in SHAPES])
def test_scan_workspace_and_plan_with_the_flag(shape):
    lib = _capi.load()
    *dims, family, base = shape
    B, KD, L, N = dims[:4]
    plain, det = bwd_params(*dims), bwd_params(*dims, flags=_capi.SIGMA_SCAN_BWD_DETERMINISTIC)
    p0, p1 = (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 6)()
    assert lib.sigma_scan_bwd_plan(ctypes.byref(plain), ctypes.byref(p0)) == 0, _capi.last_error()
    assert lib.sigma_scan_bwd_plan(ctypes.byref(det), ctypes.byref(p1)) == 0, _capi.last_error()
    assert list(p0) == list(p1), "determinism must not move the kernel choice"
    assert family_of(list(p0)) == family
    assert lib.sigma_scan_bwd_workspace_bytes(ctypes.byref(plain)) == base
    segments = segments_of(list(p0))
    rows = B * segments * KD * (N + 2) * 4             # one slot of dA[N], dD, ddelta_bias per (batch, segment)
    assert lib.sigma_scan_bwd_workspace_bytes(ctypes.byref(det)) >= base + rows


def test_scan_refuses_unknown_flag_bits():
    lib = _capi.load()
    bp = bwd_params(*SHAPES[0][:9], flags=2)
    assert lib.sigma_scan_bwd_workspace_bytes(ctypes.byref(bp)) < 0
    assert "flags" in _capi.last_error()


def _dw(B, d, H, W, flags):
    p = _capi.DwConvParams()
    p.batch, p.channels, p.height, p.width, p.n_orders, p.flags = B, d, H, W, 2, flags
    return p


def test_dwconv_and_colscale_workspace_queries():
    lib = _capi.load()
    det = _capi.SIGMA_DWCONV_DETERMINISTIC
    # encoder stage 0 of the 480 x 640 step: 120 x 160 planes, 32 x 32 tiles (4 x 5 per plane)
    assert lib.sigma_dwconv3x3_silu_bwd_workspace_bytes(ctypes.byref(_dw(16, 192, 120, 160, 0))) == 0
    assert lib.sigma_dwconv3x3_silu_bwd_workspace_bytes(ctypes.byref(_dw(16, 192, 120, 160, det))) == 16 * 20 * 192 * 40
    # a plane that fits LDS: one slot per (batch, channel)
    assert lib.sigma_dwconv3x3_silu_bwd_workspace_bytes(ctypes.byref(_dw(2, 64, 15, 20, det))) == 2 * 64 * 40
    assert lib.sigma_dwconv3x3_silu_bwd_workspace_bytes(ctypes.byref(_dw(2, 64, 15, 20, 2))) < 0
    # colscale: one row of C floats per block (256 / (C / 4) rows per block iteration, at most 512 blocks)
    assert lib.sigma_colscale_bwd_workspace_bytes(1000, 96) == 100 * 96 * 4
    assert lib.sigma_colscale_bwd_workspace_bytes(10 ** 6, 96) == 512 * 96 * 4
    assert lib.sigma_colscale_bwd_workspace_bytes(1000, 97) < 0


# ------------------------------------------------------------------------------------------------------- static ISA
ATOMIC = re.compile(r"^\s+(global_atomic|flat_atomic|buffer_atomic)\w*")
ISA_TEXT = {}          # file -> its whole assembly listing, filled by the `isa` fixture
ISA_FILES = ["scan_bwdr.hip", "scan_bwd.hip", "scan_bwd2.hip", "scan_bwd3.hip", "scan_bwd4.hip", "dwconv.hip", "pointwise.hip"]


def _functions(lines):
    """{demangled name: body lines} of every kernel in an assembly listing"""
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+):", l)] if m]
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in starts), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for (i, _), name in zip(starts, names):
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        out[name] = lines[i:end]
    return out


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    from sigma_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip(f"no hipcc at {build.HIPCC}")
    if shutil.which("c++filt") is None:
        pytest.skip("no c++filt")
    d = tmp_path_factory.mktemp("isa_det")
    flags = [f for f in build.FLAGS if f != "-fPIC"]

    def one(src):
        out = d / src.replace(".hip", ".s")
        subprocess.check_call([build.HIPCC, *flags, "--offload-device-only", "-S", os.path.join(build.CSRC, src), "-o", str(out)],
                              stderr=subprocess.DEVNULL)
        ISA_TEXT[src] = out.read_text()
        return _functions(ISA_TEXT[src].split("\n"))

    with cf.ThreadPoolExecutor(len(ISA_FILES)) as ex:
        funcs = {}
        for f in ex.map(one, ISA_FILES):
            funcs.update(f)
    return funcs


def _atomics(body):
    return [l.strip() for l in body if ATOMIC.match(l)]


# (pattern of the deterministic kernels, pattern of the default kernels they stand in for)
PAIRS = [
    (r"scan_bwdr_kernel<\d, 3>", r"scan_bwdr_kernel<\d, 0>"),
    (r"scan_bwd_det_kernel<", r"scan_bwd_kernel<"),
    (r"scan_bwd2_det_kernel<", r"scan_bwd2_kernel<"),
    (r"scan_bwd3_det_kernel<", r"scan_bwd3_kernel<"),
    (r"scan_bwd4_det_kernel<", r"scan_bwd4_kernel<"),
    (r"dwconv_silu_bwd1_det_kernel\(", r"dwconv_silu_bwd1_kernel\("),
    (r"dwconv_silu_bwd_plane_det_kernel\(", r"dwconv_silu_bwd_plane_kernel\("),
    (r"colscale_bwd_part_kernel\(", r"colscale_bwd_kernel\("),
]


@pytest.mark.parametrize("det_pat,default_pat", PAIRS, ids=[p[0].split("<")[0].split("\\")[0] for p in PAIRS])
def test_deterministic_kernels_issue_no_float_atomics(isa, det_pat, default_pat):
    det = {n: b for n, b in isa.items() if re.search(det_pat, n)}
    default = {n: b for n, b in isa.items() if re.search(default_pat, n)}
    assert det and default, (det_pat, default_pat)
    for name, body in det.items():
        assert not _atomics(body), f"{name}: {_atomics(body)[:3]}"
    for name, body in default.items():              # the default instantiations keep their atomics (they are unchanged)
        assert any("global_atomic_add_f32" in a or "global_atomic_pk_add" in a for a in _atomics(body)), name


def test_loss_family_is_340_kernels_without_scratch(isa):
    """pointwise.hip instantiates the loss kernels that are launched and no other -- 17 regimes (16 register rows and the
    walking kernel) x 2 pitches x 2 directions x (1 plain + 2 option + 2 focal, without and with class weights) -- and none
    of them keeps its row, or anything else, in scratch memory"""
    kernels = re.findall(r"^\t\.amdhsa_kernel (_ZN\S*softmax_\S+)\n(.*?)^\t\.end_amdhsa_kernel", ISA_TEXT["pointwise.hip"], re.M | re.S)
    assert len(kernels) == len({n for n, _ in kernels}) == 340 == 17 * 2 * 2 * 5
    assert sum(1 for n in isa if "softmax_" in n) == 340
    for name, desc in kernels:
        (size,) = re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", desc)
        assert int(size) == 0 and ".amdhsa_uses_dynamic_stack 0" in desc, name


def test_deterministic_row_lane_backward_keeps_the_counted_wait(isa):
    from tests.test_isa_waits_cpu import check_counted_wait
    found = 0
    for ns in (1, 2, 4):
        (body,) = [b for n, b in isa.items() if f"scan_bwdr_kernel<{ns}, 3>" in n]
        check_counted_wait(body)
        found += 1
    assert found == 3


# ------------------------------------------------------------------------------------------------------- the switch
def test_switch_follows_torch_flag_and_contract():
    import warnings
    import torch
    import sigma_amd
    from sigma_amd.deterministic import no_deterministic_implementation
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        assert sigma_amd.deterministic_enabled()
        with pytest.raises(RuntimeError, match="does not have a deterministic implementation"):
            no_deterministic_implementation("some_op")
        torch.use_deterministic_algorithms(True, warn_only=True)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            no_deterministic_implementation("some_op")
        assert any("does not have a deterministic implementation" in str(x.message) for x in w)
        torch.use_deterministic_algorithms(False)
        assert not sigma_amd.deterministic_enabled()
    finally:
        torch.use_deterministic_algorithms(was)


def test_environment_opt_in_sets_the_torch_flags():
    import sys
    code = ("import torch, sigma_amd; print(torch.are_deterministic_algorithms_enabled(), "
            "torch.utils.deterministic.fill_uninitialized_memory, sigma_amd.deterministic_enabled())")
    for val, want in (("1", "True False True"), ("0", "False True False")):
        env = dict(os.environ, SIGMA_DETERMINISTIC=val)
        out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, env=env, text=True).split("\n")[-2]
        assert out == want, (val, out)


def test_deterministic_cross_entropy_equals_torch():
    """the loss the small models use in deterministic mode (class counts the HIP kernel does not take)"""
    import torch
    from sigma_amd.pointwise import cross_entropy_deterministic
    crit = torch.nn.CrossEntropyLoss(reduction="mean", ignore_index=255)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 9, 5, 7, generator=g, dtype=torch.float64, requires_grad=True)
    lab = torch.randint(0, 9, (2, 5, 7), generator=g)
    lab[0, :2] = 255
    a, b = crit(x, lab), cross_entropy_deterministic(crit, x, lab)
    torch.testing.assert_close(b, a)
    torch.testing.assert_close(torch.autograd.grad(b, x)[0], torch.autograd.grad(a, x)[0])
