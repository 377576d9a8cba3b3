"""Child processes of tests/test_tuned_gemms_gpu.py: TunableOp state is process-wide, so everything that enables it runs
here.  Tuning itself stays OFF in both modes (look-up only, as in the product).

``rows <dir>``: the committed table switched on exactly as bench.py does (sigma_amd.tuning.enable_tuned_gemms), untuned
recording into <dir>; every row of the table on every operand regime of tests/tuned_gemm_cases.py plus the Gaussian one
three times on the same operands.  One line ``[row] <json>`` per row; one row's operands are live at a time.  Exit 3:
PyTorch rejected the table (the differing validator is printed); exit 4: a row raised -- nothing runs after it.

``census <batch> <dir>``: TunableOp on with an EMPTY table and untuned recording into <dir>, then one forward + backward
of sigma_small 480x640, 40 classes, train(): every vendor GEMM misses, so the untuned file lists what the step issues.
The GEMM mode comes from the environment (SIGMA_GEMM)."""
import glob
import json
import os
import sys
import time

import torch

UNTUNED_ENV = "PYTORCH_TUNABLEOP_UNTUNED_FILENAME"


def read_untuned(directory):
    """PyTorch inserts the device ordinal into the file name: read whatever the directory holds"""
    from tests.tuned_gemm_cases import untuned_signatures
    out = set()
    for path in glob.glob(os.path.join(directory, "untuned*")):
        with open(path) as f:
            out |= untuned_signatures(f.read())
    return out


def run_rows(directory) -> int:
    import torch.cuda.tunable as tun
    from sigma_amd.tuning import enable_tuned_gemms, table_path, tuned_gemms_active
    from tests import tuned_gemm_cases as tc
    os.environ[UNTUNED_ENV] = os.path.join(directory, "untuned.csv")
    assert enable_tuned_gemms(), "the lookup was not switched on (SIGMA_TUNED_GEMMS=0 in the environment?)"
    tun.record_untuned_enable(True)
    assert tun.is_enabled() and not tun.tuning_is_enabled() and tun.record_untuned_is_enabled()
    validators, rows, problems = tc.parse_table(table_path())
    assert not problems, problems
    dev = torch.device("cuda", 0)
    probe = torch.ones(8, 8, device=dev)
    torch.mm(probe, probe)                                   # TunableOp reads the table at the first GEMM
    torch.cuda.synchronize()
    if not tuned_gemms_active():
        mine = dict((v[0], v[1]) for v in tun.get_validators())
        diff = [f"{k}: file {validators.get(k)!r}, this stack {mine.get(k)!r}" for k in sorted(set(mine) | set(validators))
                if mine.get(k) != validators.get(k)]
        print(f"[rejected] PyTorch did not accept {table_path()}: {'; '.join(diff) or 'no validator differs'}", flush=True)
        return 3
    seen = read_untuned(directory)
    print("[header] " + json.dumps(dict(active=True, results=len(tun.get_results()), rows=len(rows), probe_untuned=sorted(map(list, seen)))),
          flush=True)
    t_all = time.time()
    for index, row in enumerate(rows):
        rec = dict(i=index, op=row.op, sig=row.signature, unit=tc.is_unit(row), regimes={})
        t0 = time.time()
        try:
            for regime in tc.REGIMES:
                A, B = tc.make_operands(regime, row, tc.seed_of(index, regime), device=dev)
                ref, scale = tc.reference(A, B), tc.abs_product(A, B)
                call = tc.prepare(row, A, B)
                got = call()
                assert got.shape == ref.shape and got.dtype == torch.float32, (got.shape, got.dtype)
                err = (got.double() - ref).abs()
                if regime in tc.EXACT_REGIMES:
                    rec["regimes"][regime] = dict(precondition=float(scale.max()), equal=bool(torch.equal(got.double(), ref)),
                                                  wrong=int((err != 0).sum()), max_err=float(err.max()))
                else:
                    bound = tc.gauss_gamma(row.k) * scale
                    again = [call(), call()]
                    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, float("inf"), 0.0).double())
                    rec["regimes"][regime] = dict(finite=bool(torch.isfinite(got).all()), within=bool((err <= bound).all()),
                                                  ratio=float(ratio.max()), repeats=bool(all(torch.equal(got, g) for g in again)))
                    del again, bound, ratio
                del A, B, ref, scale, call, got, err
            torch.cuda.synchronize()
        except Exception as e:                               # noqa: BLE001 -- reported, and nothing more runs on the GPU
            rec["error"] = repr(e)[:2000]
            print("[row] " + json.dumps(rec), flush=True)
            return 4
        now = read_untuned(directory)
        rec["missed"] = sorted(list(s) for s in now - seen if "_float_" in s[0])
        seen = now
        rec["ms"] = round(1e3 * (time.time() - t0), 1)
        print("[row] " + json.dumps(rec), flush=True)
    assert tun.is_enabled() and not tun.tuning_is_enabled() and tuned_gemms_active()
    print(f"[rows] done {len(rows)} rows in {time.time() - t_all:.1f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB", flush=True)
    return 0


def run_census(batch: int, directory) -> int:
    import torch.cuda.tunable as tun
    os.environ[UNTUNED_ENV] = os.path.join(directory, "untuned.csv")
    tun.set_filename(os.path.join(directory, "empty_table.csv"))     # never written: no results, no write on exit
    tun.tuning_enable(False)
    if hasattr(tun, "write_file_on_exit"):
        tun.write_file_on_exit(False)
    tun.record_untuned_enable(True)
    tun.enable(True)
    from sigma_amd.gemm import gemm_mode
    from sigma_amd.tuning import tuned_gemms_requested
    from tests.model_utils import build_model, fill
    H, W, classes = 480, 640, 40
    t0 = time.time()
    model = build_model("sigma_small", classes, H, W).cuda().train()
    rgb, x, label = fill.make_inputs(batch, H, W, classes, seed=3)
    loss = model(rgb.cuda(), x.cuda(), label.cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    assert not tuned_gemms_requested() and not tun.tuning_is_enabled() and len(tun.get_results()) == 0
    print(f"[census] done batch {batch} mode {gemm_mode()}: {len(read_untuned(directory))} signatures in {time.time() - t0:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "rows":
        sys.exit(run_rows(sys.argv[2]))
    sys.exit(run_census(int(sys.argv[2]), sys.argv[3]))
