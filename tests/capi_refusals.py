"""A refusal of the C ABI, asserted with its reason.

The library has one error text per thread for all three headers (``_capi.last_error``), written by every refusal and
by no success.  ``assert_refused`` therefore poisons the text first with an unrelated, host-only scan refusal: a
refusal that does not write its own reason leaves the poison behind and fails.  Nothing here touches a device --
every refusal happens on the host before any launch.
"""
from __future__ import annotations

from sigma_amd import _capi


def _poison() -> str:
    assert _capi.load().sigma_scan_set_option(b"no_such_option", 1) != 0
    text = _capi.last_error()
    assert text, "the scan refusal that poisons the error text left it empty"
    return text


def assert_refused(fn, *args, code=1, says=None, msg=None):
    """``fn(*args)`` returns `code` (default SIGMA_OPS_ERR_ARG; -1 for a size query) and leaves a reason of its own in
    the error text: non-empty, not the poison written just before, and containing `says` where given.  `msg` labels a
    failure (the case of a loop).  Returns the reason."""
    poison = _poison()
    rc = int(fn(*args))
    text = _capi.last_error()
    assert rc == code, (msg, rc, text)
    assert text and text != poison, (msg, "the refusal left no reason of its own", text)
    if says is not None:
        assert says in text, (msg, says, text)
    return text
