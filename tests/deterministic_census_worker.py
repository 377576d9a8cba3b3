"""Child process of tests/test_stream_fp64_gpu.py::test_census_of_the_deterministic_step: one forward + backward of
sigma_small (480x640, batch 2) and of sigma_base (720x1280, batch 1) under torch.use_deterministic_algorithms(True,
warn_only=True) -- torch's own non-deterministic ops (the odd-size F.interpolate of sigma_base) warn instead of stopping
the census -- with every stream-kernel, GEMM and scan call keyed by the recorder of the census.  Prints one line
``[census] <model> <repr of the sorted keys>`` per model."""
import sys

import torch


def main() -> int:
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = False
    from sigma_amd import deterministic_enabled
    from tests.test_stream_fp64_gpu import CENSUS_MODELS, _census, recording
    assert deterministic_enabled()
    with recording() as log:
        for name, H, W, batch, classes in CENSUS_MODELS:
            print(f"[census] {name} {_census(name, H, W, batch, classes, log)!r}", flush=True)
    print("[deterministic_census_worker] done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
