"""tests/tuned_gemm_cases.py without a GPU: the committed TunableOp table is sound (and a corrupted copy is refused), the
operand generators keep their exactness preconditions at every K of the table, the exact regimes see the errors they are
there for (reference code only), and the builder's operands carry the strides the row's signature states."""
import os

import pytest
import torch

from tests import tuned_gemm_cases as tc

VALIDATORS, ROWS, PROBLEMS = tc.parse_table()
BY_K = {}
for _i, _r in enumerate(ROWS):
    BY_K.setdefault(_r.k, (_i, _r))


def _representatives():
    """smallest K, largest K, one batched row, one unit-dimension row"""
    plain = [(i, r) for i, r in enumerate(ROWS) if not tc.is_unit(r)]
    small = min(plain, key=lambda t: (t[1].k, t[1].m * t[1].n * (t[1].batch or 1)))
    large = max(plain, key=lambda t: t[1].k)
    batched = min((t for t in plain if t[1].batch and t[1].batch > 1 and t[1].k > 64), key=lambda t: t[1].m * t[1].n * t[1].k * t[1].batch)
    unit = next((i, r) for i, r in enumerate(ROWS) if tc.is_unit(r) and r.k > 1)
    return [small, large, batched, unit]


REPRESENTATIVES = _representatives()


# ---------------------------------------------------------------------------------------------------- table integrity
def test_table_is_sound():
    assert tc.table_problems(VALIDATORS, ROWS, PROBLEMS) == []
    assert set(VALIDATORS) == set(tc.VALIDATORS)
    assert len(ROWS) == 595 and len({(r.op, r.signature) for r in ROWS}) == 595
    assert {r.op for r in ROWS} == set(tc.OP_KINDS)
    assert sum(tc.is_unit(r) for r in ROWS) == 48
    assert all(tc.unit_kind(r) is not None for r in ROWS if tc.is_unit(r))        # each one is a GEMM of the (1, C) MLP
    assert max(r.k for r in ROWS) == 614400 and max(r.batch or 1 for r in ROWS) == 64


def test_table_path_is_the_products():
    from sigma_amd.tuning import table_path
    assert os.path.samefile(table_path(), tc.TABLE)


def test_corrupted_copy_is_refused(tmp_path):
    """one row repeated under another solution, one row with a zero dimension, one validator gone, one foreign solution"""
    lines = open(tc.TABLE).read().splitlines()
    first = lines[5].split(",")
    zero = lines[6].split(",")
    sig = zero[1].split("_")
    sig[2] = "0"
    bad = [l for l in lines if "ROCBLAS_VERSION" not in l]
    bad.append(",".join([first[0], first[1], "Gemm_Rocblas_1", "0.5"]))
    bad.append(",".join([zero[0], "_".join(sig), zero[2], zero[3]]))
    bad.append("GemmTunableOp_float_NN,nn_8_8_8_ld_8_8_8,Gemm_Cutlass_3,0.1")
    bad.append("GemmTunableOp_float_NN,nn_8_8_ld_8_8_8,Default,0.1")
    path = tmp_path / "table.csv"
    path.write_text("\n".join(bad) + "\n")
    problems = tc.table_problems(*tc.parse_table(str(path)))
    assert len(problems) == 5, problems
    text = "\n".join(problems)
    for needle in ("ROCBLAS_VERSION is missing", f"({first[0]},{first[1]}): repeats line 5", "a dimension is not positive",
                   "Gemm_Cutlass_3", "does not parse"):
        assert needle in text, (needle, problems)


# ------------------------------------------------------------------------------------------------ generator guarantees
@pytest.mark.parametrize("K", sorted(BY_K), ids=lambda k: f"K{k}")
def test_generators_keep_their_preconditions(K):
    """4 rows and columns at the full K (and the full batch): integer entries, |A| @ |B| < 2^24 in the exact regimes, the
    stated ranges, densities and scales"""
    index, row = BY_K[K]
    for regime in tc.REGIMES:
        A, B = tc.make_operands(regime, row, tc.seed_of(index, regime), rows=4, cols=4)
        sa, sb = tc.logical_shapes(row)
        assert A.shape == sa[:-2] + (min(4, row.m), K) and B.shape == sb[:-2] + (K, min(4, row.n))
        assert A.dtype == B.dtype == torch.float32
        A2, B2 = tc.make_operands(regime, row, tc.seed_of(index, regime), rows=4, cols=4)
        assert torch.equal(A, A2) and torch.equal(B, B2)                          # a function of the seed
        if regime == "gauss":
            assert torch.isfinite(A).all() and torch.isfinite(B).all()
            assert torch.isfinite(tc.abs_product(A, B).float()).all()             # no fp32 overflow even with every sign aligned
            assert 0 < tc.gauss_gamma(K) < 0.04
            continue
        assert torch.equal(A, A.round()) and torch.equal(B, B.round())
        assert float(tc.abs_product(A, B).max()) < 2 ** 24
        ref = tc.reference(A, B)
        assert torch.equal(ref.float().double(), ref)                             # the reference itself is an fp32 value
        if regime == "dense_int":
            r = tc.dense_int_range(K)
            assert 1 <= r <= 64 and K * r * r < 2 ** 24 and (r == 64 or K * (r + 1) ** 2 >= 2 ** 24)
            assert float(A.abs().max()) <= r and float(B.abs().max()) <= r
        else:
            wide, ones = (A, B) if regime == "wide_a" else (B.transpose(-1, -2), A)
            assert torch.equal(ones.abs(), torch.ones_like(ones))
            nz = wide != 0
            assert torch.equal(nz.sum(-1), torch.full(wide.shape[:-1], min(K, tc.WIDE_NNZ)))
            assert torch.equal(wide[nz].abs() % 2, torch.ones_like(wide[nz])) and float(wide.abs().max()) <= tc.WIDE_MAX
            assert bool(nz.reshape(-1, K)[0, -1])
            if min(K, tc.WIDE_NNZ) * wide.shape[:-1].numel() >= 256:
                assert float(wide.abs().max()) >= 2048                            # 12 significant bits are in use


def test_dense_int_range_at_the_largest_k():
    assert tc.dense_int_range(614400) == 5 and tc.dense_int_range(96) == 64 and tc.dense_int_range(4096) == 63


# --------------------------------------------------------------------------------------------------- negative controls
STRUCTURAL = ("k_tail_dropped", "last_batch_from_first", "lda_off_by_one")
PRECISION = ("bf16_operands", "11bit_operands")


@pytest.mark.parametrize("index,row", REPRESENTATIVES, ids=[f"{r.op[:-9]}-{r.signature}" for _, r in REPRESENTATIVES])
def test_exact_regimes_see_the_planted_errors(index, row):
    """Reference code only.  At most 16 rows and columns of the row's operands and the full K and batch (a defect seen in
    a crop is seen in the whole).  Every exact regime must differ from every indexing defect; both wide-mantissa roles
    must differ from both operand roundings.  dense_int holds 7-bit integers, which bf16 and an 11-bit significand keep,
    so it is REQUIRED to be blind there: the precision claim rests on the wide-mantissa regime alone."""
    for regime in tc.EXACT_REGIMES:
        A, B = tc.make_operands(regime, row, tc.seed_of(index, regime), rows=16, cols=16)
        ref = tc.reference(A, B)
        wrong = tc.planted_errors(row, A, B)
        assert set(PRECISION) <= set(wrong)
        if row.k > 1:
            assert "k_tail_dropped" in wrong
        if row.batch:
            assert "last_batch_from_first" in wrong
        if A.shape[-2] > 1 and row.k > 1:
            assert "lda_off_by_one" in wrong
        for name, bad in wrong.items():
            assert bad.shape == ref.shape
            if name in STRUCTURAL or regime != "dense_int":
                assert not torch.equal(bad, ref), f"{regime} does not see {name} at {row.signature}"
            else:
                assert torch.equal(bad, ref), f"{regime} sees {name}: its entries are wider than stated"


def test_round_significand_is_bf16():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(5)) * 1000
    assert torch.equal(tc.round_significand(x, 8).float(), x.bfloat16().float())
    assert torch.equal(tc.round_significand(torch.tensor([2049.0, 4095.0, 2047.0]), 11), torch.tensor([2048.0, 4096.0, 2047.0]).double())


# --------------------------------------------------------------------------------------------------- builder self-check
def _fake_operands(row):
    sa, sb = tc.logical_shapes(row)
    return torch.empty(sa, device="meta"), torch.empty(sb, device="meta")


@pytest.mark.parametrize("kind", tc.OP_KINDS)
def test_builder_states_the_rows_signature(kind):
    """meta tensors (no storage): for every non-unit row the placed operands have the logical shapes, the transposes and
    leading dimensions of the signature, and ATen's own rule turns them back into the row's signature string"""
    rows = [r for r in ROWS if r.op == kind and not tc.is_unit(r)]
    assert rows
    for row in rows:
        A, B = _fake_operands(row)
        a, b = tc.place(row, A, B)
        assert a.shape == A.shape and b.shape == B.shape
        ta, tb = row.layout[1] == "t", row.layout[0] == "t"
        assert a.stride()[-2:] == ((1, row.lda) if ta else (row.lda, 1))
        assert b.stride()[-2:] == ((1, row.ldb) if tb else (row.ldb, 1))
        if row.batch is not None:
            assert a.stride(0) == row.lda * (row.k if ta else row.m) and b.stride(0) == row.ldb * (row.n if tb else row.k)
        assert tc.aten_signature(a, b) == row.signature
        assert row.ldc == row.n                                                   # mm / bmm allocate a dense result


def test_builder_places_values_where_the_view_says():
    """a small row of each layout at a padded pitch, on real storage: the views equal the logical operands and mm on them
    equals the reference"""
    for layout in ("nn", "nt", "tn", "tt"):
        for batch in (None, 3):
            m, n, k = 5, 7, 6
            ta, tb = layout[1] == "t", layout[0] == "t"
            lda, ldb = (m if ta else k) + 2, (k if tb else n) + 3
            row = tc.Row("x", layout, m, n, k, batch, lda, ldb, n, "Default", 0.0, "", 0)
            A, B = tc.make_operands("dense_int", row, 7)
            a, b = tc.place(row, A, B)
            assert torch.equal(a, A) and torch.equal(b, B)
            assert a.stride()[-2:] == ((1, lda) if ta else (lda, 1)) and b.stride()[-2:] == ((1, ldb) if tb else (ldb, 1))
            assert torch.equal(tc.prepare(row, A, B)().double(), tc.reference(A, B))


def test_unit_rows_are_the_mlp_calls():
    """every unit-dimension row through F.linear on a (1, C) row and its autograd backward equals A @ B, from contiguous
    x (1, in), W (out, in) and dy (1, out) as the squeeze/excite MLP holds them"""
    for index, row in enumerate(ROWS):
        if not tc.is_unit(row):
            continue
        kind, cin, cout = tc.unit_kind(row)
        for regime in tc.EXACT_REGIMES:
            A, B = tc.make_operands(regime, row, tc.seed_of(index, regime))
            x, W, dy = tc.unit_operands(row, A, B)
            # ATen takes a leading dimension from the strides even of a dimension of size 1: those of a fresh tensor
            assert x.shape == (1, cin) and x.stride() == (cin, 1) and W.shape == (cout, cin) and W.stride() == (cin, 1)
            assert (dy is None) == (kind == "forward") and (dy is None or (dy.shape == (1, cout) and dy.stride() == (cout, 1)))
            got = tc.prepare(row, A, B)()
            assert got.shape == (row.m, row.n) and torch.equal(got.double(), tc.reference(A, B))


def test_untuned_file_reader():
    text = "GemmTunableOp_float_NN,nn_8_8_8_ld_8_8_8\nGemmTunableOp_double_NN,nn_8_8_8_ld_8_8_8,extra\n\n"
    assert tc.untuned_signatures(text) == {("GemmTunableOp_float_NN", "nn_8_8_8_ld_8_8_8"), ("GemmTunableOp_double_NN", "nn_8_8_8_ld_8_8_8")}
