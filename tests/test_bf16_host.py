"""CPU: the 16-bit feature entry point (gnnagg_gcn_run_typed) is declared, exported and typed; Aggregator_GCN.run refuses feature
dtypes other than float32 / bfloat16 before it touches the device; without a GPU the typed call returns an error instead of computing."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_dtypes_and_the_typed_entry_point():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    assert re.search(r"^#define GNNAGG_DTYPE_F32 0\b", text, re.M) and re.search(r"^#define GNNAGG_DTYPE_BF16 1\b", text, re.M)
    assert re.search(r"int gnnagg_gcn_run_typed\(gnnagg_handle h, const void \*d_x, int x_dtype, void \*d_y, int y_dtype, int feat, "
                     r"int mode, int reduce,\s+int flags\);", text)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "gnnagg_gcn_run_typed" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert (_lib.DTYPE_F32, _lib.DTYPE_BF16) == (0, 1)
    res, args = _lib.SIGNATURES["gnnagg_gcn_run_typed"]
    assert res is ctypes.c_int and args == [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert gnc.lib().gnnagg_gcn_run_typed.argtypes == args


class _NoDevice(Exception):
    pass


def _handleless_aggregator(monkeypatch, V=4):
    """an Aggregator_GCN without a device handle, whose every library call raises _NoDevice"""
    agg = gnc.Aggregator_GCN.__new__(gnc.Aggregator_GCN)
    agg.num_v, agg.num_e, agg.feat_in, agg.feat_out, agg._h = V, 0, 8, 8, ctypes.c_int64(0)

    def no_device():
        raise _NoDevice()
    monkeypatch.setattr(gnc.aggregator, "lib", no_device)
    monkeypatch.setattr(gnc.aggregator.Aggregator, "_use_current_stream", lambda self: no_device())
    return agg


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_run_rejects_other_feature_dtypes_before_any_launch(monkeypatch, dtype):
    agg = _handleless_aggregator(monkeypatch)
    other, f32, b16 = torch.zeros((4, 8), dtype=dtype), torch.zeros((4, 8)), torch.zeros((4, 8), dtype=torch.bfloat16)
    for vin, vout in ((other, f32), (f32, other), (other, b16), (b16, other)):
        with pytest.raises(TypeError, match="float32 or torch.bfloat16"):
            agg.run(vin, vout, 512, "balanced")
        with pytest.raises(TypeError):
            gnc.gcn_run(agg, vin, vout, 512, 1)
    # float32 and bfloat16 pass the dtype gate and reach the library (here: the stub)
    for vin, vout in ((b16, f32), (b16, b16), (f32, b16), (f32, f32)):
        with pytest.raises(_NoDevice):
            agg.run(vin, vout, 512, "balanced")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_typed_call_errors_out_without_a_gpu():
    L = gnc.lib()
    x = np.zeros(8, np.uint16)
    y = np.zeros(8, np.float32)
    for xt, yt in ((_lib.DTYPE_BF16, _lib.DTYPE_F32), (_lib.DTYPE_BF16, _lib.DTYPE_BF16), (_lib.DTYPE_F32, _lib.DTYPE_BF16), (7, 0)):
        rc = L.gnnagg_gcn_run_typed(ctypes.c_int64(0), x.ctypes.data, xt, y.ctypes.data, yt, 8, _lib.MODE_BALANCED, _lib.REDUCE_SUM, 0)
        assert rc == _lib.ERR_ARG and b"handle" in L.gnnagg_last_error()
    ptr, idx = np.array([0, 1], np.int32), np.array([0], np.int32)
    h = ctypes.c_int64(0)
    assert L.gnnagg_gcn_create(ptr.ctypes.data, idx.ctypes.data, None, 1, 1, ctypes.byref(h)) == _lib.ERR_HIP and h.value == 0
