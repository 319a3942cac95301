"""CPU: the typed aggregation + dense combine (gnnagg_gcn_run_with_nn_typed) and gnnagg_last_nn_path are declared, exported and typed; every
dtype combination outside (f32 | bf16, f32, f32, f32) and (f32 | bf16, bf16, bf16, f32 | bf16), a NULL operand, feat_out < 1 and
GNNAGG_FLAG_ACCUMULATE are refused before the handle is used; Aggregator_GCN.run_with_nn_typed checks dtypes and shapes before it reaches
the library."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
NAME = {F32: "fp32", BF16: "bf16"}
ACCEPTED = [(x, y, w, t) for x in (F32, BF16) for (y, w, t) in ((F32, F32, F32), (BF16, BF16, F32), (BF16, BF16, BF16))]
REFUSED = [c for c in itertools.product((F32, BF16), repeat=4) if c not in ACCEPTED]


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    assert re.search(r"int gnnagg_gcn_run_with_nn_typed\(gnnagg_handle h, const void \*d_x, int x_dtype, void \*d_y, int y_dtype,\s*"
                     r"const void \*d_weight, int w_dtype,\s*void \*d_transformed, int t_dtype,\s*int feat, int feat_out, int mode, "
                     r"int reduce, int flags\);", text)
    assert re.search(r"int gnnagg_last_nn_path\(gnnagg_handle h, int \*path\);", text)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"gnnagg_gcn_run_with_nn_typed", "gnnagg_last_nn_path"} <= exported
    i, p = ctypes.c_int, ctypes.c_void_p
    res, args = _lib.SIGNATURES["gnnagg_gcn_run_with_nn_typed"]
    assert res is i and args == [ctypes.c_int64, p, i, p, i, p, i, p, i, i, i, i, i, i]
    assert gnc.lib().gnnagg_gcn_run_with_nn_typed.argtypes == args
    res, args = _lib.SIGNATURES["gnnagg_last_nn_path"]
    assert res is i and args == [ctypes.c_int64, ctypes.POINTER(ctypes.c_int)]
    assert gnc.lib().gnnagg_last_nn_path.argtypes == args


def _call(combo, feat=8, feat_out=4, flags=0, null=None, handle=0):
    """the typed call on dummy host pointers and a handle that does not exist: only argument checks may run"""
    L = gnc.lib()
    buf = np.zeros(64, np.float32)
    ptr = [buf.ctypes.data] * 4
    if null is not None:
        ptr[null] = None
    rc = L.gnnagg_gcn_run_with_nn_typed(handle, ptr[0], combo[0], ptr[1], combo[1], ptr[2], combo[2], ptr[3], combo[3], feat, feat_out,
                                        _lib.MODE_BALANCED, _lib.REDUCE_SUM, flags)
    return rc, L.gnnagg_last_error().decode()


def test_the_table_has_six_accepted_and_ten_refused_combinations():
    assert len(ACCEPTED) == 6 and len(REFUSED) == 10


@pytest.mark.parametrize("combo", REFUSED)
def test_other_dtype_combinations_are_refused_by_name_before_the_handle(combo):
    rc, msg = _call(combo)
    assert rc == _lib.ERR_ARG and "gnnagg_gcn_run_with_nn_typed" in msg, msg
    for what, t in zip(("x", "y", "weight", "transformed"), combo):
        assert "%s %s" % (what, NAME[t]) in msg, msg
    assert "handle" not in msg


def test_unknown_dtype_codes_are_refused():
    for pos in range(4):
        combo = [F32] * 4
        combo[pos] = 7
        rc, msg = _call(combo)
        assert rc == _lib.ERR_ARG and "gnnagg_gcn_run_with_nn_typed" in msg and "7" in msg, msg


@pytest.mark.parametrize("combo", ACCEPTED)
def test_sizes_null_operands_and_accumulate_are_refused_before_the_handle(combo):
    for kw in (dict(feat_out=0), dict(feat_out=-3), dict(feat=0), dict(null=0), dict(null=1), dict(null=2), dict(null=3),
               dict(flags=_lib.FLAG_ACCUMULATE), dict(flags=_lib.FLAG_ACCUMULATE | _lib.FLAG_RELU)):
        rc, msg = _call(combo, **kw)
        assert rc == _lib.ERR_ARG and "gnnagg_gcn_run_with_nn_typed" in msg and "handle" not in msg, (kw, msg)
        for what, t in zip(("x", "y", "weight", "transformed"), combo):
            assert "%s %s" % (what, NAME[t]) in msg, msg
    rc, msg = _call(combo, flags=_lib.FLAG_ACCUMULATE)
    assert "GNNAGG_FLAG_ACCUMULATE" in msg
    # everything else in order: the handle is what is missing (no device is touched; this machine may have none)
    for flags in (0, _lib.FLAG_RELU):
        rc, msg = _call(combo, flags=flags)
        assert rc == _lib.ERR_ARG and "handle" in msg, msg


def test_last_nn_path_needs_a_handle():
    L = gnc.lib()
    p = ctypes.c_int(-1)
    assert L.gnnagg_last_nn_path(0, ctypes.byref(p)) == _lib.ERR_ARG and "handle" in L.gnnagg_last_error().decode()
    assert p.value == -1


class _NoDevice(Exception):
    pass


@pytest.fixture
def agg(monkeypatch):
    """an Aggregator_GCN of 4 rows whose every way into the library raises"""
    def no_device():
        raise _NoDevice()
    monkeypatch.setattr(gnc.aggregator, "lib", no_device)
    a = object.__new__(gnc.Aggregator_GCN)
    a.num_v, a.num_e, a._h = 4, 0, ctypes.c_int64(0)
    return a


def _t(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_run_with_nn_typed_rejects_other_dtypes_before_the_library(agg, dtype):
    b = torch.bfloat16
    good = [_t((4, 8), b), _t((4, 8), b), _t((8, 3), b), _t((4, 3), b)]
    shapes = [(4, 8), (4, 8), (8, 3), (4, 3)]
    for pos in range(4):
        ops = list(good)
        ops[pos] = _t(shapes[pos], dtype)
        with pytest.raises(TypeError, match="float32 or torch.bfloat16"):
            agg.run_with_nn_typed(*ops)
    with pytest.raises(TypeError):
        agg.run_with_nn_typed(good[0], good[1], good[2], np.zeros((4, 3), np.float32))


def test_run_with_nn_typed_rejects_combinations_outside_the_table_before_the_library(agg):
    f, b = torch.float32, torch.bfloat16
    for x, y, w, t in ((f, f, b, f), (f, b, f, f), (b, f, f, b), (f, f, f, b), (b, b, f, b), (b, f, b, b)):
        with pytest.raises(TypeError, match="run_with_nn_typed"):
            agg.run_with_nn_typed(_t((4, 8), x), _t((4, 8), y), _t((8, 3), w), _t((4, 3), t))


def test_run_with_nn_typed_rejects_mismatched_shapes_before_the_library(agg):
    b = torch.bfloat16
    for vin, vout, w, t in ((_t((4, 8), b), _t((4, 8), b), _t((7, 3), b), _t((4, 3), b)),      # weight rows != F
                            (_t((4, 8), b), _t((4, 7), b), _t((8, 3), b), _t((4, 3), b)),      # vout too small
                            (_t((4, 8), b), _t((4, 8), b), _t((8, 3), b), _t((4, 2), b)),      # transformed too small
                            (_t((3, 8), b), _t((4, 8), b), _t((8, 3), b), _t((4, 3), b)),      # vin has fewer rows than the graph
                            (_t((32,), b), _t((4, 8), b), _t((8, 3), b), _t((4, 3), b)),       # vin not [V, F]
                            (_t((4, 8)), _t((4, 8)), _t((8,)), _t((4, 3)))):                   # weight not [F, N]
        with pytest.raises(ValueError):
            agg.run_with_nn_typed(vin, vout, w, t)
    with pytest.raises(ValueError):
        agg.run_with_nn_typed(_t((4, 8)), _t((4, 8)), _t((8, 3)), _t((4, 3)), reduce="median")


def test_run_with_nn_typed_reaches_the_library_with_the_accepted_combinations(agg):
    f, b = torch.float32, torch.bfloat16
    for x in (f, b):
        for y, w, t in ((f, f, f), (b, b, f), (b, b, b)):
            for relu in (False, True):
                with pytest.raises(_NoDevice):
                    agg.run_with_nn_typed(_t((4, 8), x), _t((4, 8), y), _t((8, 3), w), _t((4, 3), t), relu=relu)
    with pytest.raises(_NoDevice):
        agg.last_nn_path()
