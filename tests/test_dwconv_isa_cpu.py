"""gfx950 ISA of csrc/dwconv.hip (no GPU): no kernel may spill.  The run kernels hold a 3 x 6 window, the weights, ten
sums and (backward) the row-major gradient of up to six runs in registers through fully unrolled loops; an index the
compiler cannot resolve at compile time would put those arrays into scratch memory, at a large cost and with no failing
test.  Compiled the way tests/test_deterministic_cpu.py compiles its listings."""
import os
import re
import subprocess

import pytest


def test_no_dwconv_kernel_uses_scratch(tmp_path):
    from sigma_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip(f"no hipcc at {build.HIPCC}")
    out = tmp_path / "dwconv.s"
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    subprocess.check_call([build.HIPCC, *flags, "--offload-device-only", "-S", os.path.join(build.CSRC, "dwconv.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    # one .amdhsa_kernel ... .end_amdhsa_kernel descriptor block per kernel
    blocks = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)
    sizes = {name: int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) for name, body in blocks}
    dw = {n: s for n, s in sizes.items() if "dwconv" in n}
    assert len(dw) >= 7, sorted(sizes)          # forward, bwd1 (2), bwd2, whole-plane backward (2), reduce
    assert all(s == 0 for s in dw.values()), {n: s for n, s in dw.items() if s}
