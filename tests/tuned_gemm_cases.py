"""The committed TunableOp table (sigma_amd/tuning/tunableop_mi355x.csv) as test cases: a parser with integrity checks,
a builder that makes ATen issue exactly a row's signature, and three operand regimes with an fp64 reference.  Imports on
the CPU and takes nothing from sigma_amd but the table's path; tests/test_tuned_gemms_cpu.py checks this module without
a GPU, tests/tuned_gemm_worker.py runs it on the MI355X with the lookup on (tests/test_tuned_gemms_gpu.py).

Signatures.  ATen computes the row-major C(m x n) = A(m x k) @ B(k x n) as the column-major C^T = B^T A^T, so a row
``GemmTunableOp_float_XY, xy_N_M_K_ld_LDB_LDA_LDC`` reads: x = 't' when B is a transposed view of an (n, k) row-major
matrix (leading dimension LDB), y = 't' when A is a transposed view of a (k, m) one (LDA); LDC is the row pitch of C.
The batched kind inserts ``B_<batch>`` before ``ld``.

Regimes (u = 2^-24; every generator takes a seed and a device):

* ``dense_int``: integers in [-r, r], r = min(64, floor(sqrt((2^24 - 1) / K))).  Every partial sum in any order is an
  integer of magnitude <= K r^2 < 2^24, so a correct fp32 GEMM is bit-exact.  Sees indexing: a dropped K tail, a wrong
  leading dimension, wrong batch strides.  Its values fit 7 bits, so it cannot see operand rounding (bf16 holds them).
* ``wide_a`` / ``wide_b``: one operand has min(K, 1024) non-zeros along K per row (one at a random place in each of
  that many equal chunks of K; row 0 always has one at K - 1), odd integers up to 4095 with random sign = 12 significant
  bits; the other is dense +-1.  max(|A| @ |B|) <= 1024 * 4095 = 4 193 280 < 2^24 by construction, so the result is
  again bit-exact for fp32 operands and an fp32 accumulator, and not for bf16 / 11-bit operands.
* ``gauss``: standard normal entries, rows of A and columns of B scaled by 2^e, e in [-40, 40].  For fp32 products
  summed in fp32 in ANY order (Higham, Accuracy and Stability, (3.5) with n = K + 2 roundings to cover an FMA-free
  product and the alpha / beta epilogue): |got - ref| <= g (|A| @ |B|), g = (K + 2) u / (1 - (K + 2) u).  Products stay
  within 2^-100 .. 2^100 except where two entries below 2^-10 meet at the smallest scales; a flush there moves an element by
  2^-126, below one ulp of the bound.
"""
from __future__ import annotations

import collections
import math
import os
import re

import torch
import torch.nn.functional as F

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sigma_amd", "tuning", "tunableop_mi355x.csv")
VALIDATORS = ("PT_VERSION", "HIP_VERSION", "HIPBLASLT_VERSION", "GCN_ARCH_NAME", "ROCBLAS_VERSION")
OP_KINDS = tuple(f"GemmTunableOp_float_{l}" for l in ("NN", "NT", "TN", "TT")) + \
    tuple(f"GemmStridedBatchedTunableOp_float_{l}" for l in ("NN", "NT", "TN"))
EXACT_REGIMES = ("dense_int", "wide_a", "wide_b")
REGIMES = EXACT_REGIMES + ("gauss",)
U = 2.0 ** -24
WIDE_NNZ = 1024
WIDE_MAX = 4095

Row = collections.namedtuple("Row", "op layout m n k batch lda ldb ldc solution time signature lineno")
_SIG = re.compile(r"^([nt]{2})_(\d+)_(\d+)_(\d+)(?:_B_(\d+))?_ld_(\d+)_(\d+)_(\d+)$")
_SOLUTION = re.compile(r"^(Default|Gemm_Rocblas_-?\d+|Gemm_Hipblaslt_-?\d+)$")


# ------------------------------------------------------------------------------------------------------------ the table
def parse_table(path=TABLE):
    """-> (validators {name: value}, rows [Row], problems [str]).  A line that does not parse becomes a problem, not a row."""
    validators, rows, problems = {}, [], []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split(",")
            if parts[0] == "Validator":
                if len(parts) != 3 or parts[1] in validators:
                    problems.append(f"line {lineno}: bad or repeated validator: {line}")
                else:
                    validators[parts[1]] = parts[2]
                continue
            m = _SIG.match(parts[1]) if len(parts) == 4 else None
            if m is None:
                problems.append(f"line {lineno}: does not parse: {line}")
                continue
            try:
                time = float(parts[3])
            except ValueError:
                problems.append(f"line {lineno}: time is not a number: {line}")
                continue
            layout, n, mm, k, batch, ldb, lda, ldc = m.groups()
            rows.append(Row(parts[0], layout, int(mm), int(n), int(k), None if batch is None else int(batch), int(lda), int(ldb),
                            int(ldc), parts[2], time, parts[1], lineno))
    return validators, rows, problems


def table_problems(validators, rows, problems=()):
    """every way the table breaks what the tests (and PyTorch's reader) rely on; [] for a sound table"""
    out = list(problems)
    out += [f"validator {v} is missing" for v in VALIDATORS if v not in validators]
    seen = {}
    for r in rows:
        where = f"line {r.lineno} ({r.op},{r.signature})"
        if r.op not in OP_KINDS:
            out.append(f"{where}: unknown op kind")
        elif r.op.rsplit("_", 1)[1].lower() != r.layout:
            out.append(f"{where}: layout of the signature differs from the op's")
        elif ("Batched" in r.op) != (r.batch is not None):
            out.append(f"{where}: batch field does not fit the op kind")
        if min(r.m, r.n, r.k, r.lda, r.ldb, r.ldc, 1 if r.batch is None else r.batch) <= 0:
            out.append(f"{where}: a dimension is not positive")
        else:
            ta, tb = r.layout[1] == "t", r.layout[0] == "t"
            if r.lda < (r.m if ta else r.k) or r.ldb < (r.k if tb else r.n) or r.ldc < r.n:
                out.append(f"{where}: a leading dimension is shorter than its row")
        if not _SOLUTION.match(r.solution):
            out.append(f"{where}: solution {r.solution!r} is neither Default nor a rocBLAS / hipBLASLt one")
        if not (r.time >= 0 and math.isfinite(r.time)):
            out.append(f"{where}: time {r.time}")
        if (r.op, r.signature) in seen:
            out.append(f"{where}: repeats line {seen[r.op, r.signature]}")
        seen.setdefault((r.op, r.signature), r.lineno)
    return out


def is_unit(row) -> bool:
    return 1 in (row.m, row.n, row.k)


# ---------------------------------------------------------------------------------------------------------- the builder
def logical_shapes(row):
    """shapes of A and B in C = A @ B"""
    b = () if row.batch is None else (row.batch,)
    return b + (row.m, row.k), b + (row.k, row.n)


def _pitched(x, transposed, ld):
    """x (..., r, c) copied into storage whose rows have pitch ld, as a view of the same shape; with ``transposed`` the
    storage holds x^T (c rows of pitch ld) and the view is its transpose"""
    src = x.transpose(-1, -2) if transposed else x
    store = torch.zeros(src.shape[:-1] + (ld,), dtype=x.dtype, device=x.device)
    store[..., :src.shape[-1]].copy_(src)
    view = store[..., :src.shape[-1]]
    return view.transpose(-1, -2) if transposed else view


def place(row, A, B):
    """A, B (logical, any strides) -> views with the strides the row's signature states"""
    return _pitched(A, row.layout[1] == "t", row.lda), _pitched(B, row.layout[0] == "t", row.ldb)


def aten_signature(a, b):
    """the signature ATen's mm / bmm issues for these operands (at::native prepare_matrix_for_cublas /
    prepare_batch_matrix_for_cublas: a matrix whose columns have stride 1 goes in as it is, one whose rows have stride 1
    as its transpose, anything else is copied first -> None here); no dimension may be 1"""
    m, k, n = a.shape[-2], a.shape[-1], b.shape[-1]
    assert b.shape[-2] == k and min(m, n, k) > 1

    def one(x):
        rows, cols = x.shape[-2:]
        sr, sc = x.stride()[-2:]
        if sc == 1 and sr >= max(1, cols):
            return "n", sr
        if sr == 1 and sc >= max(1, rows):
            return "t", sc
        return None

    pa, pb = one(a), one(b)
    if pa is None or pb is None:
        return None
    batch = "" if a.dim() == 2 else f"_B_{a.shape[0]}"
    if a.dim() == 3 and (a.stride(0) < a.shape[1] * a.shape[2] or b.stride(0) < b.shape[1] * b.shape[2]):
        return None                                       # an expanded batch is materialised by bmm
    return f"{pb[0]}{pa[0]}_{n}_{m}_{k}{batch}_ld_{pb[1]}_{pa[1]}_{n}"


def unit_kind(row):
    """a unit-dimension row as the squeeze/excite MLP issues it at batch 1: which GEMM of y = F.linear(x, W), x (1, in),
    W (out, in) it is -> (kind, in, out)"""
    if row.batch is None and row.m == 1 and row.layout == "tn":
        return "forward", row.k, row.n                    # y = x W^T
    if row.batch is None and row.m == 1 and row.layout == "nn":
        return "grad_x", row.n, row.k                     # dx = dy W
    if row.batch is None and row.k == 1 and row.layout == "nn":
        return "grad_w", row.n, row.m                     # dW = dy^T x
    return None


def _fresh(x, shape):
    """x in new storage of this shape with the strides of a freshly made tensor: ATen reads a leading dimension off the
    strides even where the dimension is 1 and .contiguous() would keep whatever stride a view had there"""
    return torch.empty(shape, dtype=x.dtype, device=x.device).copy_(x.reshape(shape))


def unit_operands(row, A, B):
    """logical A, B of a unit row -> (x, W, dy) of the F.linear call; dy is None for the forward"""
    kind, cin, cout = unit_kind(row)
    if kind == "forward":
        return _fresh(A, (1, cin)), _fresh(B.t(), (cout, cin)), None
    if kind == "grad_x":
        return torch.ones(1, cin, dtype=A.dtype, device=A.device), _fresh(B, (cout, cin)), _fresh(A, (1, cout))
    return _fresh(B, (1, cin)), torch.zeros(cout, cin, dtype=A.dtype, device=A.device), _fresh(A, (1, cout))


def prepare(row, A, B):
    """-> a callable that issues the row's GEMM on A, B (placed once: calling it again repeats the very same GEMM)"""
    if is_unit(row):
        kind = unit_kind(row)
        if kind is None:
            raise NotImplementedError(f"no product call known for {row.op},{row.signature}")
        x, W, dy = unit_operands(row, A, B)
        if kind[0] == "forward":
            return lambda: F.linear(x, W)
        x.requires_grad_(kind[0] == "grad_x")
        W.requires_grad_(kind[0] == "grad_w")
        leaf = x if kind[0] == "grad_x" else W
        return lambda: torch.autograd.grad(F.linear(x, W), leaf, dy)[0]
    a, b = place(row, A, B)
    return (lambda: torch.mm(a, b)) if row.batch is None else (lambda: torch.bmm(a, b))


# ---------------------------------------------------------------------------------------------------------- the regimes
def dense_int_range(K: int) -> int:
    return min(64, math.isqrt((2 ** 24 - 1) // K))


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def _signs(shape, g, device):
    return (torch.randint(0, 2, shape, generator=g, device=device) * 2 - 1).float()


def _wide(lead, K, g, device):
    """(*lead, K) fp32: min(K, 1024) odd integers of up to 12 bits per row, one in each equal chunk of K"""
    nnz = min(K, WIDE_NNZ)
    vals = (torch.randint(0, (WIDE_MAX + 1) // 2, lead + (nnz,), generator=g, device=device) * 2 + 1).float() * _signs(lead + (nnz,), g, device)
    if nnz == K:
        return vals
    edges = torch.arange(nnz + 1, device=device, dtype=torch.int64) * K // nnz
    start, length = edges[:-1], edges[1:] - edges[:-1]
    off = (torch.rand(lead + (nnz,), generator=g, device=device, dtype=torch.float64) * length).long().clamp_(max=length - 1)
    pos = start + off
    pos.reshape(-1, nnz)[0, -1] = K - 1                   # the K tail is seen in at least one row
    return torch.zeros(lead + (K,), device=device).scatter_(-1, pos, vals)


def make_operands(regime, row, seed, device="cpu", rows=None, cols=None):
    """-> logical A (.., m, k), B (.., k, n) in fp32.  ``rows`` / ``cols`` crop m / n (the CPU checks keep the full K)."""
    m = row.m if rows is None else min(rows, row.m)
    n = row.n if cols is None else min(cols, row.n)
    K, lead = row.k, (() if row.batch is None else (row.batch,))
    g = _gen(seed, device)
    if regime == "dense_int":
        r = dense_int_range(K)
        A = torch.randint(-r, r + 1, lead + (m, K), generator=g, device=device).float()
        B = torch.randint(-r, r + 1, lead + (K, n), generator=g, device=device).float()
    elif regime == "wide_a":
        A, B = _wide(lead + (m,), K, g, device), _signs(lead + (K, n), g, device)
    elif regime == "wide_b":
        A, B = _signs(lead + (m, K), g, device), _wide(lead + (n,), K, g, device).transpose(-1, -2)
    elif regime == "gauss":
        ea = torch.randint(-40, 41, lead + (m, 1), generator=g, device=device)
        eb = torch.randint(-40, 41, lead + (1, n), generator=g, device=device)
        A = torch.ldexp(torch.randn(lead + (m, K), generator=g, device=device), ea)
        B = torch.ldexp(torch.randn(lead + (K, n), generator=g, device=device), eb)
    else:
        raise ValueError(regime)
    return A, B


def reference(A, B):
    return A.double() @ B.double()


def abs_product(A, B):
    """|A| @ |B| in fp64: the exactness precondition of the integer regimes (max < 2^24) and the scale of the bound"""
    return A.abs().double() @ B.abs().double()


def gauss_gamma(K: int) -> float:
    return (K + 2) * U / (1 - (K + 2) * U)


def seed_of(index: int, regime: str) -> int:
    return 20240 + len(REGIMES) * index + REGIMES.index(regime)


# --------------------------------------------------------------------------------------- planted errors (reference code)
def round_significand(x, bits):
    """x (fp32 / fp64) rounded to ``bits`` significant bits, to nearest even (bits = 8: bf16 for values in its range)"""
    mant, exp = torch.frexp(x.double())
    return torch.ldexp(torch.round(mant * 2.0 ** bits) / 2.0 ** bits, exp)


def planted_errors(row, A, B):
    """{name: fp64 product a defective GEMM of this row would give}; a name is left out where the row has no such defect
    (a single batch, a result too small for a pitch error)"""
    out = {
        "bf16_operands": round_significand(A, 8) @ round_significand(B, 8),
        "11bit_operands": round_significand(A, 11) @ round_significand(B, 11),
    }
    Ad, Bd = A.double(), B.double()
    if row.k > 1:
        out["k_tail_dropped"] = Ad[..., :-1] @ Bd[..., :-1, :]
    if row.batch is not None and row.batch > 1:
        out["last_batch_from_first"] = torch.cat([Ad[:-1], Ad[:1]]) @ Bd
    if A.shape[-2] > 1 and row.k > 1:
        # A read at pitch k + 1 from its own dense storage: element (i, j) comes from flat index i (k + 1) + j
        flat = torch.cat([Ad.reshape(Ad.shape[:-2] + (-1,)), Ad.new_zeros(Ad.shape[:-2] + (A.shape[-2],))], -1)
        idx = (torch.arange(A.shape[-2]).unsqueeze(1) * (row.k + 1) + torch.arange(row.k)).to(A.device)
        out["lda_off_by_one"] = flat[..., idx] @ Bd
    return out


# ------------------------------------------------------------------------------------------------------- census records
def untuned_signatures(text: str):
    """lines of a TunableOp untuned file -> {(op, signature)}"""
    out = set()
    for line in text.splitlines():
        parts = line.strip().split(",")
        if len(parts) >= 2 and parts[0]:
            out.add((parts[0], parts[1]))
    return out
