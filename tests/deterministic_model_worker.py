"""Child process of tests/test_deterministic_gpu.py::test_fixture_models_match_the_reference_under_the_flag: the fixture
comparison of tests/test_model_gpu.py::test_logits_loss_and_grads_match_reference_fixtures (both fixtures, the
split-operand GEMMs of SIGMA_GEMM=split3 set by the parent, automatic checkpoint pitch, the same tolerances) under
torch.use_deterministic_algorithms(True), so that the deterministic scan / dwconv / colscale / GEMM paths and the
deterministic cross entropy are checked for VALUES against the reference's own model."""
import sys

import torch


def main() -> int:
    torch.use_deterministic_algorithms(True)
    from sigma_amd import deterministic_enabled
    from tests.model_utils import compare_with_reference_fixtures
    assert deterministic_enabled()
    for case in ("tiny_64x96", "tiny_72x88_b2"):
        compare_with_reference_fixtures(case, "split3")
        print(f"[deterministic_model_worker] {case} ok", flush=True)
    print("[deterministic_model_worker] done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
