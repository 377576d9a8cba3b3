"""Operands whose split-operand GEMM result is known EXACTLY, and the reference that computes it (no GPU needed).

Contract of the kernels (include/sigma_gemm.h, csrc/gemm_split.hip split_pair and the MFMA loop):

    piece[0] = bf16(x),  piece[q + 1] = bf16(x - piece[0] - ... - piece[q])           (round to nearest even)
    C = sum over k and over the piece pairs with qa + qb < pieces of  a_piece[qa] * b_piece[qb]   (fp32 accumulation)

The operands built here are integer valued, with every piece known and non-trivial (lo, and mid, are nonzero), such that
every kept product is a multiple of one power-of-two ``unit`` and, per output element,

    sum |kept terms| + |bias| + |residuals| + |old C|  <  2^24 units.

Every partial sum, in any order, is then a multiple of the unit below 2^24 of them, i.e. representable in fp32: whatever
the accumulation order, slice count, stage (two-stage or atomics) or tile shape, the kernel must return the reference
BIT FOR BIT.  The one hardware assumption: an MFMA returns the exact sum when every addend and partial sum is
representable (sigma_gemm_selftest relies on the same).

Nothing here trusts the construction: ``pieces_of`` applies the header's formula, ``exact_operand`` asserts that the
pieces add up to the operand and that the last one is not all zero, ``unit_of`` derives the unit from the pieces and
``assert_window`` checks the 2^24 window per output element in fp64 -- a case outside the window is a broken test
(AssertionError), never a skipped one.  The reference sums the kept products in fp64, which is exact while
sum |terms| < 2^53 (asserted too); tests/test_gemm_exact_cpu.py compares it with int64 arithmetic.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math

import torch

NAN = float("nan")
WINDOW = 2 ** 24

# value families (a nonzero element is s * magnitude, s = +-1); see exact_operand
KINDS = ("unit", "wide", "three")


def pieces_of(x: torch.Tensor, P: int):
    """the P bf16 pieces of an fp32 tensor by the header's formula (as fp32 tensors)"""
    assert x.dtype == torch.float32
    r, out = x.clone(), []
    for _ in range(P):
        h = r.to(torch.bfloat16).to(torch.float32)
        out.append(h)
        r = r - h
    return out


def exact_operand(shape, pieces: int, seed: int, density: float = 1.0, kind: str | None = None) -> torch.Tensor:
    """fp32 CPU tensor of integer values whose bf16 pieces are known and non-trivial:
        unit   s * (1024 + l), l in {-1, 0, 1}                      -> (s 1024, s l)          products <= 1026 units of 2^10
        wide   s * (1024 p + q), p in {2, 3}, |q| <= 3              -> (s 1024 p, s q)        more distinct values, K <~ 1800
        three  s * (2^18 + {512, 768} + {0, 1})                     -> (s 2^18, s {512, 768}, s {0, 1})   three pieces
    hi + lo stays inside the binade of hi (2^18 - 2^9 - 1 would round to 255 * 2^10).  ``density``: share of nonzero elements."""
    kind = kind or ("three" if pieces == 3 else "wide")
    assert kind in KINDS and (kind == "three") == (pieces == 3), (kind, pieces)
    g = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    ri = lambda lo, hi: torch.randint(lo, hi, (n,), generator=g, dtype=torch.int64)
    s = ri(0, 2) * 2 - 1
    if kind == "unit":
        mag = 1024 + ri(-1, 2)
    elif kind == "wide":
        mag = 1024 * ri(2, 4) + ri(-3, 4)
    else:
        mag = 2 ** 18 + 512 + 256 * ri(0, 2) + ri(0, 2)
    v = s * mag
    if density < 1.0:
        v = v * (torch.rand(n, generator=g) < density)
    x = v.to(torch.float32).reshape(shape)
    assert torch.equal(x.to(torch.int64).reshape(-1), v), "operand values must be exact in fp32"
    ps = pieces_of(x, pieces)
    assert torch.equal(sum(p.double() for p in ps), x.double()), "the pieces must add up to the operand"
    assert all(bool((p != 0).any()) for p in ps) or not bool((x != 0).any()), "every piece must be non-trivial"
    return x


def _lowbit(p: torch.Tensor) -> int:
    """largest power of two dividing every nonzero element of an integer-valued tensor (0: all zero)"""
    v = p.double().abs()
    assert bool((v == v.round()).all()) and float(v.max() if v.numel() else 0) < 2 ** 62
    v = v.to(torch.int64)
    v = v[v != 0]
    return int((v & -v).min()) if v.numel() else 0


def unit_of(pa, pb) -> int:
    """the power of two that divides every kept product a_piece[qa] * b_piece[qb], qa + qb < P"""
    P = len(pa)
    ua, ub = [_lowbit(p) for p in pa], [_lowbit(p) for p in pb]
    units = [ua[qa] * ub[qb] for qa in range(P) for qb in range(P - qa) if ua[qa] and ub[qb]]
    return min(units) if units else 1


def _mm(form: str, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """per-problem product in the form's orientation: nt (Z,M,K)x(Z,N,K), nn (Z,M,K)x(Z,K,N), tn (Z,T,N)x(Z,T,K)"""
    if form == "nt":
        return torch.matmul(a, b.transpose(-1, -2))
    if form == "nn":
        return torch.matmul(a, b)
    return torch.matmul(a.transpose(-1, -2), b)


def kept_products(form: str, A: torch.Tensor, B: torch.Tensor, pieces: int, a_mod: int = 0, pairs=None):
    """(sum, sum of magnitudes, unit) of the kept piece products per problem, fp64, shape (Z, rows of C, columns of C).
    A: (Za, ., .) with Za = a_mod or Z, B: (Z, ., .).  ``pairs``: override of the kept (qa, qb) set (sensitivity controls)."""
    Z = B.shape[0]
    if a_mod > 0:
        A = A[torch.arange(Z, device=A.device) % a_mod]
    pa, pb = pieces_of(A, pieces), pieces_of(B, pieces)
    unit = unit_of(pa, pb)
    pa, pb = [p.double() for p in pa], [p.double() for p in pb]
    if pairs is None:
        # sum_qa a[qa] (sum_{qb < P - qa} b[qb]): the same multiset of products, all exact in fp64
        tot = sum(_mm(form, pa[qa], sum(pb[:pieces - qa])) for qa in range(pieces))
        mag = sum(_mm(form, pa[qa].abs(), sum(p.abs() for p in pb[:pieces - qa])) for qa in range(pieces))
    else:
        tot = sum(_mm(form, pa[qa], pb[qb]) for qa, qb in pairs)
        mag = sum(_mm(form, pa[qa].abs(), pb[qb].abs()) for qa, qb in pairs)
    return tot, mag, unit


def fold_outputs(x: torch.Tensor, batch: int, c_mod: int) -> torch.Tensor:
    """(Z, M, N) per-problem values -> per-output values: problems z with the same z % c_mod are summed when batch > c_mod"""
    if not (c_mod > 0 and batch > c_mod):
        return x
    out = torch.zeros((c_mod,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    out.index_add_(0, torch.arange(batch, device=x.device) % c_mod, x)
    return out


def assert_window(mag: torch.Tensor, unit: int, what: str = "") -> float:
    """per output element: sum of |terms| below 2^24 units (every fp32 partial sum exact) and below 2^53 (the fp64
    reference exact).  Returns the worst fill of the window."""
    worst = float(mag.max()) if mag.numel() else 0.0
    assert worst < 2.0 ** 53, f"{what}: sum |terms| {worst:.3e} is not exact in fp64"
    assert worst / unit < WINDOW, f"{what}: sum |terms| = {worst / unit:.0f} units of {unit}: outside the 2^24 window, results would round"
    return worst / unit / WINDOW


def exact_product(form, A, B, pieces, *, a_mod=0, c_mod=0, bias=None, residuals=(), old=None, pairs=None, what=""):
    """The exact result (fp64, (outputs, M, N)) of one launch: kept products, problems sharing an output summed, + bias
    (every row; once per output that the bias reaches: the kernels refuse a bias on summed launches), + residuals (per
    problem), + old C (accumulate).  Asserts the window.  Returns (C, unit, window fill)."""
    Z = B.shape[0]
    tot, mag, unit = kept_products(form, A, B, pieces, a_mod, pairs)
    for r in residuals:
        tot, mag = tot + r.double(), mag + r.double().abs()
    tot, mag = fold_outputs(tot, Z, c_mod), fold_outputs(mag, Z, c_mod)
    if bias is not None:
        tot, mag = tot + bias.double(), mag + bias.double().abs()
    if old is not None:
        tot, mag = tot + old.double(), mag + old.double().abs()
    for extra in (bias, old) + tuple(residuals):
        assert extra is None or bool((extra.double() / unit == (extra.double() / unit).round()).all()), f"{what}: addend off the unit grid"
    fill = assert_window(mag, unit, what)
    return tot, unit, fill


def unit_multiples(shape, unit: int, seed: int, span: int = 2000) -> torch.Tensor:
    """fp32 integer multiples of `unit` in [-span, span] units: bias, residuals and old contents of C"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-span, span + 1, tuple(shape), generator=g, dtype=torch.int64) * unit).to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# guard bands (shared with tests/test_gemm_gpu.py)

def guarded(n, margin, fill=NAN, device="cuda"):
    """(buffer, view of n floats inside it): the margins on both sides (>= one row + 64 floats, multiples of 4 so that the
    view stays 16-byte aligned) belong to the same allocation, so a store past either end of the view lands in memory the
    test owns and is detected afterwards instead of faulting"""
    assert margin % 4 == 0
    buf = torch.full((n + 2 * margin,), fill, device=device)
    return buf, buf[margin:margin + n]


def margins_intact(buf, n, margin):
    if buf.is_cuda:
        torch.cuda.synchronize()
    head, tail = buf[:margin], buf[margin + n:]
    return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())


# ---------------------------------------------------------------------------------------------------------------------
# cases: one launch through the C ABI, laid out inside poisoned buffers

@dataclasses.dataclass(frozen=True)
class Case:
    """One launch.  M, N, K as in sigma_gemm_params (tn: M tokens, C is N x K).  ``variant``: the instantiation the case is
    meant for, (tile width, residual variant) -- tests/test_gemm_exact_cpu.py fails when the planner says otherwise."""
    name: str
    form: str
    M: int
    N: int
    K: int
    pieces: int = 2
    variant: tuple = (128, False)
    kind: str | None = None
    density: tuple = (1.0, 1.0)
    batch: int = 1
    a_mod: int = 0
    c_mod: int = 0
    bias: bool = False
    res: int = 0                 # residual tensors (0, 1, 2)
    accumulate: bool = False
    t_cols: int = 0
    k_slices: int = 0
    ws: str = "query"            # summed launches: "query" = the scratch the query asks for, "none", "short" = one byte less
    pad: tuple = (4, 8, 4, 4)    # poison columns per row of A, B, C, residuals (ld = width + pad; multiples of 4 for A, B)
    c_off: int = 0               # C starts this many floats off 16-byte alignment
    r_off: int = 0               # residuals likewise
    sC_pad: int = 0              # extra floats between the C of consecutive problems
    sR_pad: int = 0
    seed: int = 0

    # ---- geometry ---------------------------------------------------------------------------------------------------
    @property
    def a_shape(self):           # (problems of A, rows, columns)
        za = self.a_mod if self.a_mod > 0 else self.batch
        return (za, self.M, self.N) if self.form == "tn" else (za, self.M, self.K)

    @property
    def b_shape(self):
        return {"nt": (self.batch, self.N, self.K), "nn": (self.batch, self.K, self.N), "tn": (self.batch, self.M, self.K)}[self.form]

    @property
    def c_rows_cols(self):       # the full product, before t_cols splits it
        return (self.N, self.K) if self.form == "tn" else (self.M, self.N)

    @property
    def outputs(self):
        return self.c_mod if (self.c_mod > 0 and self.batch > self.c_mod) else self.batch

    @property
    def kernel_dims(self):       # rows, columns, reduction as the kernel sees them
        return (self.N, self.K, self.M) if self.form == "tn" else (self.M, self.N, self.K)

    def layout(self):
        """leading dimensions and batch strides, in floats"""
        (_, ra, ca), (_, rb, cb) = self.a_shape, self.b_shape
        rc, cc = self.c_rows_cols
        cc -= self.t_cols
        lda, ldb, ldc, ldr = ca + self.pad[0], cb + self.pad[1], cc + self.pad[2], self.c_rows_cols[1] + self.pad[3]
        return dict(lda=lda, ldb=ldb, ldc=ldc, ldr=ldr, sA=ra * lda, sB=rb * ldb, sC=rc * ldc + self.sC_pad,
                    sR=rc * ldr + self.sR_pad, ldct=rc + 4)

    def params(self, ptr):
        """sigma_gemm_params for the case; ptr: dict of addresses (A, B, C, bias, R, R2, Ct) -- real ones on the GPU, any
        16-byte aligned numbers for sigma_gemm_plan (which dereferences nothing): the offsets c_off / r_off are added here"""
        from sigma_amd import _capi
        L = self.layout()
        p = _capi.GemmParams()
        p.M, p.N, p.K = self.M, self.N, self.K
        p.A, p.Bt, p.C = ptr["A"], ptr["B"], ptr["C"] + 4 * self.c_off
        p.bias = ptr["bias"] if self.bias else None
        p.lda, p.ldb, p.ldc = L["lda"], L["ldb"], L["ldc"]
        p.accumulate, p.batch = int(self.accumulate), self.batch
        p.strideA, p.strideB, p.strideC = L["sA"], L["sB"], L["sC"]
        p.a_mod, p.pieces, p.c_mod = self.a_mod, self.pieces, self.c_mod
        if self.res:
            p.residual, p.ldr, p.strideR = ptr["R"] + 4 * self.r_off, L["ldr"], L["sR"]
            p.residual2 = ptr["R2"] + 4 * self.r_off if self.res == 2 else None
        if self.t_cols:
            p.Ct, p.ldct, p.t_cols = ptr["Ct"], L["ldct"], self.t_cols
        p.k_slices = self.k_slices
        return p

    FAKE = dict(A=0x100000, B=0x200000, C=0x300000, bias=0x400000, R=0x500000, R2=0x600000, Ct=0x700000, ws=0x800000)

    def plan(self, lib=None):
        """sigma_gemm_plan of the case as the GPU test launches it (host only): the decoded dict or None (refused)"""
        from sigma_amd import _capi
        lib = lib or _capi.load()
        p = self.params(self.FAKE)
        need = int(lib.sigma_gemm_workspace_bytes(ctypes.byref(p), _capi.GEMM_FORMS[self.form]))
        if need > 0 and self.ws != "none":
            p.workspace, p.workspace_bytes = self.FAKE["ws"], need - (1 if self.ws == "short" else 0)
        return _capi.gemm_plan(p, self.form, lib)

    # ---- operands ---------------------------------------------------------------------------------------------------
    def operands(self):
        """CPU tensors: A (Za, ., .), B (Z, ., .) and, by the unit they define, bias / residuals / old C"""
        A = exact_operand(self.a_shape, self.pieces, 1000 * self.seed + 1, self.density[0], self.kind)
        B = exact_operand(self.b_shape, self.pieces, 1000 * self.seed + 2, self.density[1], self.kind)
        unit = unit_of(pieces_of(A, self.pieces), pieces_of(B, self.pieces))
        rc, cc = self.c_rows_cols
        o = dict(A=A, B=B, unit=unit)
        o["bias"] = unit_multiples((cc,), unit, 1000 * self.seed + 3) if self.bias else None
        o["res"] = tuple(unit_multiples((self.batch, rc, cc), unit, 1000 * self.seed + 4 + i) for i in range(self.res))
        o["old"] = unit_multiples((self.outputs, rc, cc), unit, 1000 * self.seed + 7) if self.accumulate else None
        return o

    def reference(self, o, pairs=None):
        """(exact C in fp64 (outputs, rows, columns), window fill) from the operands `o` (on any device)"""
        C, unit, fill = exact_product(self.form, o["A"], o["B"], self.pieces, a_mod=self.a_mod, c_mod=self.c_mod, bias=o["bias"],
                                      residuals=o["res"], old=o["old"], pairs=pairs, what=self.name)
        assert unit == o["unit"]
        return C, fill


def poisoned(x3: torch.Tensor, ld: int, stride: int, device, off: int = 0, guard_rows: int = 2):
    """(buffer, view): the (Z, R, C) tensor x3 as a strided view (stride, ld, 1) of a NaN-filled buffer -- NaN rows before
    the first and after the last row, NaN in the columns C..ld of each row and between problems; the view starts `off`
    floats past a 16-byte boundary"""
    Z, R, C = x3.shape
    assert ld >= C and stride >= R * ld
    margin = (guard_rows * ld + 64 + 3) // 4 * 4
    n = (Z - 1) * stride + (R - 1) * ld + C
    buf = torch.full((n + 2 * margin + 4,), NAN, device=device)
    view = torch.as_strided(buf, (Z, R, C), (stride, ld, 1), margin + off)
    view.copy_(x3.to(device))
    return buf, view


def untouched_outside(buf: torch.Tensor, view: torch.Tensor) -> bool:
    """every float of `buf` outside `view` is still NaN"""
    probe = buf.clone()
    torch.as_strided(probe, view.shape, view.stride(), view.storage_offset()).fill_(NAN)
    return bool(torch.isnan(probe).all())


def run_case(case: Case, device="cuda"):
    """Launch `case` through the C ABI on operands inside poisoned buffers; returns (got, want64, report) with got the
    outputs re-assembled as (outputs, rows, columns).  Asserts the window before the launch, the return code, and that
    nothing outside the output views was written."""
    from sigma_amd import _capi, gemm
    lib = _capi.load()
    L = case.layout()
    o = case.operands()
    dev = torch.device(device)
    o_dev = dict(o, A=o["A"].to(dev), B=o["B"].to(dev), bias=None if o["bias"] is None else o["bias"].to(dev),
                 res=tuple(r.to(dev) for r in o["res"]), old=None if o["old"] is None else o["old"].to(dev))
    want, fill = case.reference(o_dev)
    rc_, cc_ = case.c_rows_cols
    T = case.t_cols
    bufA, vA = poisoned(o["A"], L["lda"], L["sA"], dev)
    bufB, vB = poisoned(o["B"], L["ldb"], L["sB"], dev)
    res_views = [poisoned(r, L["ldr"], L["sR"], dev, off=case.r_off) for r in o["res"]]
    c_init = torch.full((case.outputs, rc_, cc_ - T), NAN)
    plan = case.plan(lib)
    assert plan is not None, f"{case.name}: refused by the planner"
    if case.accumulate:
        c_init = o["old"]
    elif plan["store"] == "atomic":
        c_init = torch.zeros_like(c_init)                    # the header's contract for sums without scratch
    bufC, vC = poisoned(c_init, L["ldc"], L["sC"], dev, off=case.c_off)
    addr = lambda buf, v: buf.data_ptr() + 4 * v.storage_offset()        # (an empty view, t_cols = N, has no data_ptr of its own)
    ptr = dict(A=addr(bufA, vA), B=addr(bufB, vB), C=addr(bufC, vC) - 4 * case.c_off, bias=o_dev["bias"].data_ptr() if case.bias else 0)
    for key, (b, v) in zip(("R", "R2"), res_views):
        ptr[key] = addr(b, v) - 4 * case.r_off
    if T:
        bufT, vT = poisoned(torch.full((1, T, rc_), NAN), L["ldct"], T * L["ldct"], dev)
        ptr["Ct"] = addr(bufT, vT)
    p = case.params(ptr)
    need = int(lib.sigma_gemm_workspace_bytes(ctypes.byref(p), _capi.GEMM_FORMS[case.form]))
    ws = None
    if need > 0 and case.ws != "none":
        ws = torch.full((need // 4 + 4,), NAN, device=dev)    # the scratch is prefilled with poison too
        p.workspace, p.workspace_bytes = ws.data_ptr(), need - (1 if case.ws == "short" else 0)
    assert _capi.gemm_plan(p, case.form, lib) == plan, f"{case.name}: the plan on real addresses differs from the host-only one"
    gemm._selftest(dev)
    with torch.cuda.device(dev):
        rc = int(getattr(lib, f"sigma_gemm_{case.form}_split3")(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert rc == 0, f"{case.name}: sigma_gemm_{case.form}_split3 returned {rc}"
    torch.cuda.synchronize()
    assert untouched_outside(bufC, vC), f"{case.name}: wrote outside C"
    got = vC
    if T:
        assert untouched_outside(bufT, vT), f"{case.name}: wrote outside Ct"
        got = torch.cat([vT.transpose(1, 2), vC], dim=2)
    return got, want, dict(plan=plan, fill=fill, unit=o["unit"])


def describe_mismatch(got: torch.Tensor, want: torch.Tensor, unit: int, limit: int = 8) -> str:
    """where and by how much (in units) an exact case is off: the pattern says which tile, fragment or k-step"""
    bad = (got.double() != want) | torch.isnan(got)
    idx = bad.nonzero()
    lines = [f"{int(bad.sum())} of {bad.numel()} elements differ; NaN: {int(torch.isnan(got).sum())}; "
             f"rows {sorted(set(idx[:, 1].tolist()))[:12]} cols {sorted(set(idx[:, 2].tolist()))[:12]}"]
    for z, r, c in idx[:limit].tolist():
        lines.append(f"  [{z},{r},{c}] got {float(got[z, r, c])!r} want {float(want[z, r, c])!r} diff/unit {(float(got[z, r, c]) - float(want[z, r, c])) / unit!r}")
    return "\n".join(lines)
