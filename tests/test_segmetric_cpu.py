"""CPU checks of the evaluator's device bookkeeping (csrc/segmetric.hip, include/sigma_ops.h): the two entry points are
declared and exported, their parameter structs match gcc's layout, and the host-side checks refuse bad arguments
without touching a GPU (no refused call reaches a launch)."""
import ctypes
import os
import re
import subprocess

import pytest

from sigma_amd import _capi
from tests.capi_refusals import assert_refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_SYMBOLS = ("sigma_seg_accumulate", "sigma_seg_argmax_confusion")
ERR_ARG = 1

# stand-in device addresses: every call below is refused (or is a no-op) before anything is dereferenced
ADDR = 1 << 20


def test_entry_points_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "sigma_ops.h")).read()
    declared = set(re.findall(r"^\s*int\s+(sigma_seg_\w+)\s*\(", header, flags=re.M))
    assert declared == set(SEG_SYMBOLS)
    assert set(SEG_SYMBOLS) <= set(_capi.OPS_SYMBOLS)
    lib = _capi.load()
    for name in SEG_SYMBOLS:
        assert getattr(lib, name) is not None
    assert re.search(r"#define\s+SIGMA_SEG_LDS_HIST_BYTES\s+(\d+)", header).group(1) == str(_capi.SIGMA_SEG_LDS_HIST_BYTES)


def test_struct_layout_matches_gcc(tmp_path):
    structs = (("sigma_seg_accumulate_params", _capi.SegAccumulateParams), ("sigma_seg_confusion_params", _capi.SegConfusionParams))
    lines = []
    for cname, cls in structs:
        lines.append(f'printf("%s %zu\\n", "{cname}", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("%s.%s %zu\\n", "{cname}", "{fname}", offsetof({cname}, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigma_ops.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs:
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def _acc(**kw):
    p = _capi.SegAccumulateParams()
    p.pixels, p.classes, p.first = 12, 3, 1
    p.score, p.acc = ADDR, ADDR * 2
    p.score_plane_stride = p.acc_plane_stride = 12
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad", [dict(classes=0), dict(classes=-1), dict(classes=65536), dict(pixels=-1), dict(first=2),
                                 dict(score=None), dict(acc=None), dict(score_plane_stride=11), dict(acc_plane_stride=5),
                                 dict(score=ADDR + 2), dict(acc=ADDR * 2 + 4)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_accumulate_refuses_bad_arguments(bad):
    lib = _capi.load()
    assert_refused(lib.sigma_seg_accumulate, ctypes.byref(_acc(**bad)), None, code=ERR_ARG, says=next(iter(bad)))


def test_accumulate_null_params_and_empty_image():
    lib = _capi.load()
    assert_refused(lib.sigma_seg_accumulate, None, None, code=ERR_ARG, says="NULL")
    assert lib.sigma_seg_accumulate(ctypes.byref(_acc(pixels=0, score_plane_stride=0, acc_plane_stride=0)), None) == 0


def _conf(**kw):
    p = _capi.SegConfusionParams()
    p.pixels, p.classes, p.n_cl = 64, 9, 9
    p.gt_elem_size, p.pred_elem_size = 1, 8
    p.acc, p.acc_plane_stride = ADDR, 64
    p.pred, p.gt, p.hist, p.counts = ADDR * 2, ADDR * 3, ADDR * 4, ADDR * 5
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad", [
    dict(n_cl=0), dict(n_cl=257), dict(n_cl=-3),
    dict(classes=0), dict(classes=-1), dict(classes=65536),
    dict(pixels=-1), dict(pixels=1 << 31, acc_plane_stride=1 << 31),
    dict(gt_elem_size=2), dict(gt_elem_size=4), dict(pred_elem_size=4), dict(pred_elem_size=0),
    dict(pred_elem_size=1, classes=257),                      # a uint8 prediction cannot hold class 256
    dict(acc_plane_stride=63),
    dict(acc=ADDR + 4), dict(pred=ADDR * 2 + 4), dict(gt_elem_size=8, gt=ADDR * 3 + 1),
    dict(hist=None), dict(counts=None), dict(hist=ADDR * 4 + 4),
    dict(gt=None, pred=None),                                 # neither counts nor a prediction: nothing to do
    dict(acc=None),                                           # a given prediction needs classes == 0 ...
    dict(acc=None, classes=0, pred=None),                     # ... and the prediction itself
    dict(acc=None, classes=0, gt=None),                       # hist_info of a given prediction needs labels
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_argmax_confusion_refuses_bad_arguments(bad):
    lib = _capi.load()
    assert_refused(lib.sigma_seg_argmax_confusion, ctypes.byref(_conf(**bad)), None, code=ERR_ARG, says=next(iter(bad)))


def test_argmax_confusion_null_params_and_empty_image():
    lib = _capi.load()
    assert_refused(lib.sigma_seg_argmax_confusion, None, None, code=ERR_ARG, says="NULL")
    for kw in (dict(), dict(acc=None, classes=0), dict(gt=None, hist=None, counts=None), dict(n_cl=256, pred_elem_size=1)):
        assert lib.sigma_seg_argmax_confusion(ctypes.byref(_conf(pixels=0, **kw)), None) == 0, kw
