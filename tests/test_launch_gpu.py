"""sigma_amd/_launch.py, the torch side of every call into the library: the stream and the device a launch gets, the
error path, the pointer helper -- on sigma_pair_sum_add, the smallest launch of the C ABI (include/sigma_ops.h)."""
import pytest
import torch

from sigma_amd import _launch

pytestmark = pytest.mark.gpu


def _operands(dev):
    """src (3, 2, 8), acc (3, 8) of small integers: every sum is exact in fp32"""
    src = (torch.arange(48, device=dev, dtype=torch.float32).view(3, 2, 8) % 7) - 3
    acc = (torch.arange(24, device=dev, dtype=torch.float32).view(3, 8) % 5) * 2
    return src, acc


def _pair_sum_add(src, acc):
    _launch.launch("sigma_pair_sum_add", _launch.ptr(src), _launch.ptr(acc), 3, 8, device=src.device, what="pair_sum_add")


def test_launch_runs_on_the_current_stream():
    dev = torch.device("cuda", torch.cuda.current_device())
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        # operands produced on the side stream just before: a launch on the null stream would not be ordered after them
        src, acc = _operands(dev)
        want = acc + src.sum(1)
        _pair_sum_add(src, acc)
    side.synchronize()
    assert torch.equal(acc, want)
    src2, acc2 = _operands(dev)
    _pair_sum_add(src2, acc2)
    torch.cuda.synchronize()
    assert torch.equal(acc2, want)


def test_status_is_raised_by_launch_and_returned_by_call():
    dev = torch.device("cuda", torch.cuda.current_device())
    with pytest.raises(RuntimeError) as e:
        _launch.launch("sigma_ohem_select", None, device=dev, what="ohem_select")      # NULL params: refused before any launch
    assert str(e.value).startswith("ohem_select:") and "sigma_status 1" in str(e.value)
    assert "params is NULL" in str(e.value)                 # the reason of THIS refusal, from the library's error text
    assert _launch.call("sigma_ohem_select", None, device=dev) == 1
    src, acc = _operands(dev)
    want = acc + src.sum(1)
    _pair_sum_add(src, acc)
    torch.cuda.synchronize()
    assert torch.equal(acc, want)


def test_ptr():
    assert _launch.ptr(None) is None
    t = torch.zeros(64, device="cuda")[12:40]
    assert t.storage_offset() == 12
    assert _launch.ptr(t).value == t.data_ptr() == t.untyped_storage().data_ptr() + 48


def test_launch_on_another_device_leaves_the_current_one():
    if torch.cuda.device_count() < 2:
        pytest.skip("the device guard needs two GPUs")
    with torch.cuda.device(0):
        src, acc = _operands(torch.device("cuda", 1))
        want = acc + src.sum(1)
        _pair_sum_add(src, acc)
        assert torch.cuda.current_device() == 0
        torch.cuda.synchronize(1)
        assert torch.equal(acc, want)
