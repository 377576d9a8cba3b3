"""The committed TunableOp table on the MI355X: every row of sigma_amd/tuning/tunableop_mi355x.csv, run with the lookup
on exactly as bench.py switches it on, is exact on the integer regimes of tests/tuned_gemm_cases.py, within the fp32
theorem's bound on the scaled Gaussian one, bitwise repeatable, and really looked up (its signature never reaches the
file of signatures that MISSED the table); and every GEMM signature a training step issues that is in the table is one
of those rows.

TunableOp state is process-wide, so this process never enables it: tests/tuned_gemm_worker.py does, in four child
processes run one after the other, each under its own ``timeout -k 10``, each once per module.  A child that fails,
faults or times out fails the fixture; nothing is started after it and nothing is retried.

Measured on one MI355X: the row worker takes 13 s (595 rows x 4 regimes, fp64 references included; the limit is 300 s),
a census (process start, model build, one forward + backward with MIOpen's first-use searches) 12 s for the first and
6 s for the next two (limit 300 s each); the whole file 40 s."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests import tuned_gemm_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_LIMIT = 300
CENSUS_LIMIT = 300
# (name, batch, SIGMA_GEMM): sigma_small 480x640, 40 classes, train(), one forward + backward
CENSUS_CONFIGS = (("batch8", 8, None), ("batch8-fp32", 8, "fp32"), ("batch1", 1, None))

VALIDATORS, ROWS, PROBLEMS = tc.parse_table()
TABLE_KEYS = {(r.op, r.signature): i for i, r in enumerate(ROWS)}


def _child(args, limit, gemm_mode=None):
    env = dict(os.environ)
    env.pop("SIGMA_TUNED_GEMMS", None)                      # neither forbidden nor switched on by a constructor
    env.pop("PYTORCH_TUNABLEOP_ENABLED", None)
    env.pop("PYTORCH_TUNABLEOP_TUNING", None)
    env.pop("SIGMA_GEMM", None)
    if gemm_mode:
        env["SIGMA_GEMM"] = gemm_mode
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "tests.tuned_gemm_worker", *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=limit + 60)
    seconds = time.time() - t0
    if r.returncode != 0:
        keep = "\n".join(l for l in r.stdout.splitlines() if not l.startswith("[row] ") or '"error"' in l)
        pytest.fail(f"tuned_gemm_worker {' '.join(args)}: exit {r.returncode} after {seconds:.0f} s\n--- stdout\n{keep[-4000:]}\n"
                    f"--- stderr\n{r.stderr[-6000:]}", pytrace=False)
    return r.stdout, seconds


@pytest.fixture(scope="module")
def row_run(tmp_path_factory):
    """the row worker, once: {index: record}, the float signatures that missed the table, the header"""
    from tests.tuned_gemm_worker import read_untuned
    directory = tmp_path_factory.mktemp("tuned_rows")
    out, seconds = _child(["rows", str(directory)], ROW_LIMIT)
    records, header = {}, None
    for line in out.splitlines():
        if line.startswith("[row] "):
            rec = json.loads(line[6:])
            records[rec["i"]] = rec
        elif line.startswith("[header] "):
            header = json.loads(line[9:])
    assert "[rows] done" in out and header is not None
    probe = {tuple(s) for s in header["probe_untuned"]}
    missed = {s for s in read_untuned(str(directory)) if "_float_" in s[0]} - probe
    print(f"row worker: {seconds:.1f} s, {len(records)} rows")
    return dict(records=records, missed=missed, header=header, seconds=seconds)


def left_out(run):
    """unit-dimension rows whose F.linear call made ATen issue something else than the row (a GEMV never reaches TunableOp,
    another signature misses the table): named here, excluded from the lookup assertion only"""
    return {i for i, rec in run["records"].items() if rec["unit"] and rec["missed"]}


def row_failures(rec, run, skip_lookup=False):
    bad = []
    for regime in tc.EXACT_REGIMES:
        r = rec["regimes"][regime]
        if not r["precondition"] < 2 ** 24:
            bad.append(f"{regime}: precondition max(|A| @ |B|) = {r['precondition']}")
        if not r["equal"]:
            bad.append(f"{regime}: {r['wrong']} elements differ, max |err| {r['max_err']}")
    g = rec["regimes"]["gauss"]
    if not (g["finite"] and g["within"]):
        bad.append(f"gauss: err / bound = {g['ratio']}")
    if not g["repeats"]:
        bad.append("gauss: three runs on the same operands are not bitwise equal")
    if not skip_lookup and ((rec["op"], rec["sig"]) in run["missed"] or rec["missed"]):
        bad.append(f"missed the table: {rec['missed'] or rec['sig']}")
    return bad


def _of_kind(run, kind):
    recs = [rec for rec in run["records"].values() if rec["op"] == kind]
    assert len(recs) == sum(r.op == kind for r in ROWS) > 0
    return recs


def test_table_is_accepted_and_every_row_ran(row_run):
    """PyTorch accepted the table (the worker exits 3 and names the differing validator otherwise: a failure, not a skip,
    since bench.py would be measuring an untuned step); all 595 rows ran; rows left out of the lookup assertion are
    unit-dimension rows only, and are named"""
    assert not PROBLEMS and row_run["header"]["active"] and row_run["header"]["results"] == len(ROWS) == 595
    assert sorted(row_run["records"]) == list(range(len(ROWS)))
    for i, rec in row_run["records"].items():
        assert (rec["op"], rec["sig"]) == (ROWS[i].op, ROWS[i].signature) and "error" not in rec
    out = left_out(row_run)
    for i in sorted(out):
        print(f"left out of the lookup assertion: {ROWS[i].op},{ROWS[i].signature} (issued {row_run['records'][i]['missed']})")
    print(f"tested {len(ROWS) - len(out)} rows, left out {len(out)}")
    assert all(tc.is_unit(ROWS[i]) for i in out)


@pytest.mark.parametrize("kind", tc.OP_KINDS)
def test_rows_are_exact_on_the_integer_regimes(row_run, kind):
    bad = {rec["sig"]: [b for b in row_failures(rec, row_run, True) if b.split(":")[0] in tc.EXACT_REGIMES] for rec in _of_kind(row_run, kind)}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, bad


@pytest.mark.parametrize("kind", tc.OP_KINDS)
def test_rows_are_within_the_fp32_bound_on_scaled_gaussians(row_run, kind):
    recs = _of_kind(row_run, kind)
    worst = max(recs, key=lambda rec: rec["regimes"]["gauss"]["ratio"])
    print(f"{kind}: worst err / bound {worst['regimes']['gauss']['ratio']:.3e} at {worst['sig']}")
    bad = {rec["sig"]: rec["regimes"]["gauss"] for rec in recs if not (rec["regimes"]["gauss"]["finite"] and rec["regimes"]["gauss"]["within"])}
    assert not bad, bad


@pytest.mark.parametrize("kind", tc.OP_KINDS)
def test_rows_repeat_bitwise(row_run, kind):
    bad = [rec["sig"] for rec in _of_kind(row_run, kind) if not rec["regimes"]["gauss"]["repeats"]]
    assert not bad, bad


@pytest.mark.parametrize("kind", tc.OP_KINDS)
def test_rows_are_looked_up(row_run, kind):
    """the row's signature is absent from the signatures that missed, and its call made nothing else miss: the solution
    the table names is what ran"""
    out = left_out(row_run)
    bad = {rec["sig"]: rec["missed"] or "its own signature" for rec in _of_kind(row_run, kind)
           if rec["i"] not in out and ((rec["op"], rec["sig"]) in row_run["missed"] or rec["missed"])}
    assert not bad, bad


def test_nothing_else_missed(row_run):
    """every float signature that missed during the row worker belongs to a named left-out row"""
    named = {tuple(s) for i in left_out(row_run) for s in row_run["records"][i]["missed"]}
    assert row_run["missed"] <= named, sorted(row_run["missed"] - named)


# -------------------------------------------------------------------------------------------------------------- census
@pytest.fixture(scope="module")
def census_run(row_run, tmp_path_factory):
    """three steps under an empty table, one child each, after the row worker and only if it ended well"""
    from tests.tuned_gemm_worker import read_untuned
    issued, seconds = {}, {}
    for name, batch, mode in CENSUS_CONFIGS:
        directory = tmp_path_factory.mktemp(f"tuned_census_{name}")
        out, seconds[name] = _child(["census", str(batch), str(directory)], CENSUS_LIMIT, mode)
        assert "[census] done" in out
        issued[name] = read_untuned(str(directory))
        assert issued[name], f"census {name}: no signature recorded"
    return dict(issued=issued, seconds=seconds)


def census_report(row_run, census_run) -> str:
    lines = ["# TunableOp census: sigma_small 480x640, 40 classes, train(), one forward + backward under an empty table",
             f"# table: {len(ROWS)} rows; written by tests/test_tuned_gemms_gpu.py::test_census_hits_are_tested_rows (pytest -rP)"]
    used = set()
    for name, _, _ in CENSUS_CONFIGS:
        sigs = census_run["issued"][name]
        hits, misses = sigs & set(TABLE_KEYS), sigs - set(TABLE_KEYS)
        used |= hits
        lines.append(f"{name}: issued {len(sigs)}, hits {len(hits)}, misses {len(misses)} ({census_run['seconds'][name]:.0f} s)")
        lines += [f"  miss {op},{sig}" for op, sig in sorted(misses)]
    stale = set(TABLE_KEYS) - used
    lines.append(f"stale (rows none of the three steps issues): {len(stale)} of {len(ROWS)}")
    for kind in tc.OP_KINDS:
        lines.append(f"  {kind}: {sum(op == kind for op, _ in stale)} stale of {sum(r.op == kind for r in ROWS)}")
    lines += [f"  stale {op},{sig}" for op, sig in sorted(stale)]
    lines.append(f"row worker {row_run['seconds']:.0f} s")
    return "\n".join(lines)


def test_census_hits_are_tested_rows(row_run, census_run):
    """every signature of the three steps that is in the table is a row the row worker ran, passed on every count and
    looked up (so not a left-out row).  Misses and stale rows are reported (profiles/tuned_gemm_census.txt),
    not asserted: re-tuning is a performance change of its own."""
    print("[census report]\n" + census_report(row_run, census_run) + "\n[end of census report]")
    out = left_out(row_run)
    bad = {}
    for name, _, _ in CENSUS_CONFIGS:
        hits = census_run["issued"][name] & set(TABLE_KEYS)
        assert hits, f"{name}: the step issues no row of the table"
        for key in hits:
            i = TABLE_KEYS[key]
            fails = (["left out"] if i in out else []) + row_failures(row_run["records"][i], row_run)
            if fails:
                bad[f"{name}: {key[0]},{key[1]}"] = fails
    assert not bad, bad
