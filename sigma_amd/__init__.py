"""sigma_amd: the MI355X (gfx950) operators of the project.  See sigma_amd/deterministic.py for deterministic mode."""
import os as _os


def deterministic_enabled() -> bool:
    """True when the HIP operators run their bitwise-reproducible forms (torch.are_deterministic_algorithms_enabled())."""
    from .deterministic import enabled
    return enabled()


if _os.environ.get("SIGMA_DETERMINISTIC", "0").strip() not in ("", "0"):
    from .deterministic import enable_from_env as _enable_from_env
    _enable_from_env()
