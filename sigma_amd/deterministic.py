"""Deterministic mode: bitwise-reproducible backward passes of the project's HIP operators.

The mode follows torch's own switch: it is on while ``torch.are_deterministic_algorithms_enabled()`` is true, read at
every launch (no state is cached here).  In this mode

  * the scan backward runs with ``SIGMA_SCAN_BWD_DETERMINISTIC`` (include/sigma_scan.h): dA / dD / ddelta_bias leave
    every workgroup through plain stores into a slot of the workspace, added in a fixed order;
  * the depthwise conv backward runs with ``SIGMA_DWCONV_DETERMINISTIC`` and the decoder residual scale through
    ``sigma_colscale_bwd_ws`` (include/sigma_ops.h), both two-stage sums;
  * the split-operand GEMMs always sum their slices through the workspace (gemm.py), whatever ``SIGMA_GEMM_TWO_STAGE``
    says, and a launch that would need float atomics raises instead.

A path without a deterministic form follows torch's contract: ``RuntimeError("... does not have a deterministic
implementation ...")``, or a warning under ``torch.use_deterministic_algorithms(True, warn_only=True)``.

``SIGMA_DETERMINISTIC=1`` in the environment turns the mode on when ``sigma_amd`` is imported, for callers that cannot
edit their script (bench.py, train.py, eval.py): :func:`enable_from_env` calls ``torch.use_deterministic_algorithms(True)``
so that ATen and MIOpen follow the same rule, and sets ``torch.utils.deterministic.fill_uninitialized_memory = False``
(the NaN fill of every ``torch.empty`` is a cost a benchmark should not pay; every kernel here writes what it returns).
These two, with ``CUBLAS_WORKSPACE_CONFIG`` (set to ``:4096:8`` only when it is unset, because torch may refuse vendor
GEMMs under the flag without it), are the only global state the package touches, and only on this opt-in.
"""
from __future__ import annotations

import os
import warnings

import torch

ENV = "SIGMA_DETERMINISTIC"


def enabled() -> bool:
    """True while torch's deterministic-algorithms flag is set."""
    return torch.are_deterministic_algorithms_enabled()


def env_requested() -> bool:
    return os.environ.get(ENV, "0").strip() not in ("", "0")


def enable_from_env() -> None:
    """The ``SIGMA_DETERMINISTIC=1`` opt-in (see the module docstring)."""
    os.environ.setdefault("CUBLAS_WORKSPACE_CONFIG", ":4096:8")
    torch.use_deterministic_algorithms(True)
    torch.utils.deterministic.fill_uninitialized_memory = False


def no_deterministic_implementation(what: str) -> None:
    """torch's contract for an operation without a deterministic form: raise, or warn under ``warn_only``."""
    msg = (f"{what} does not have a deterministic implementation, but you set "
           "'torch.use_deterministic_algorithms(True)'.")
    if torch.is_deterministic_algorithms_warn_only_enabled():
        warnings.warn(msg + " (warn_only: running the non-deterministic form)")
    else:
        raise RuntimeError(msg)
