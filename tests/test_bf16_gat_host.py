"""CPU: the 16-bit feature entry point of the fused GAT aggregation (gnnagg_gat_run_typed) is declared, exported and typed;
Aggregator_GAT.run refuses feature dtypes other than float32 / bfloat16 (and attention terms / newval other than float32) before it
touches the device; without a GPU the typed call returns an error instead of computing."""
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


def test_header_declares_the_typed_gat_entry_point():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    assert re.search(r"int gnnagg_gat_run_typed\(gnnagg_handle h, const void \*d_x, int x_dtype, const float \*d_att, void \*d_y, "
                     r"int y_dtype,\s+int feat, int heads, float slope, int mode, float \*d_newval\);", text)
    assert "the GAT entry points are fp32 only" not in text
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "gnnagg_gat_run_typed" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    res, args = _lib.SIGNATURES["gnnagg_gat_run_typed"]
    assert res is ctypes.c_int and args == [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    assert gnc.lib().gnnagg_gat_run_typed.argtypes == args


class _NoDevice(Exception):
    pass


def _handleless_aggregator(monkeypatch, V=4):
    """an Aggregator_GAT without a device handle, whose every library call raises _NoDevice"""
    agg = gnc.Aggregator_GAT.__new__(gnc.Aggregator_GAT)
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
    att = torch.zeros((4, 2))
    for vin, vout in ((other, f32), (f32, other), (other, b16), (b16, other)):
        with pytest.raises(TypeError, match="float32 or torch.bfloat16"):
            agg.run(vin, att, vout, 128, "balanced")
        with pytest.raises(TypeError):
            gnc.gat_run(agg, vin, att, vout, 128, 1)
    # float32 and bfloat16 pass the dtype gate and reach the library (here: the stub)
    for vin, vout in ((b16, f32), (b16, b16), (f32, b16), (f32, f32)):
        with pytest.raises(_NoDevice):
            agg.run(vin, att, vout, 128, "balanced")
        with pytest.raises(_NoDevice):
            gnc.gat_run(agg, vin, att, vout, 128, 1)


def test_attention_terms_and_newval_stay_float32(monkeypatch):
    agg = _handleless_aggregator(monkeypatch)
    f32, b16 = torch.zeros((4, 8)), torch.zeros((4, 8), dtype=torch.bfloat16)
    att, att16 = torch.zeros((4, 2)), torch.zeros((4, 2), dtype=torch.bfloat16)
    for vin, vout in ((b16, f32), (b16, b16), (f32, b16), (f32, f32)):
        with pytest.raises(TypeError, match="vatt must be torch.float32"):
            agg.run(vin, att16, vout, 128, "balanced")
        with pytest.raises(TypeError, match="newval must be torch.float32"):
            agg.run(vin, att, vout, 128, "balanced", newval=torch.zeros(3, dtype=torch.bfloat16))
    # run_part and probe_gather keep requiring float32 features (no device: CPU tensors are refused before the dtype is looked at, so
    # the dtype refusal itself is checked on the GPU, tests/test_gpu_bf16_gat.py)
    with pytest.raises((TypeError, ValueError, _NoDevice)):
        agg.run_part(b16, att, f32, torch.zeros((4, 1)), 1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_typed_call_errors_out_without_a_gpu():
    L = gnc.lib()
    x = np.zeros(8, np.uint16)
    att = np.zeros(2, np.float32)
    y = np.zeros(8, np.float32)
    for xt, yt in ((_lib.DTYPE_BF16, _lib.DTYPE_F32), (_lib.DTYPE_BF16, _lib.DTYPE_BF16), (_lib.DTYPE_F32, _lib.DTYPE_BF16),
                   (_lib.DTYPE_F32, _lib.DTYPE_F32), (7, 0), (0, -1)):
        rc = L.gnnagg_gat_run_typed(ctypes.c_int64(0), x.ctypes.data, xt, att.ctypes.data, y.ctypes.data, yt, 8, 1, ctypes.c_float(0.2),
                                    _lib.MODE_BALANCED, None)
        assert rc == _lib.ERR_ARG and len(L.gnnagg_last_error()) > 0 and b"handle" in L.gnnagg_last_error()
    ptr, idx = np.array([0, 1], np.int32), np.array([0], np.int32)
    h = ctypes.c_int64(0)
    assert L.gnnagg_gat_create(ptr.ctypes.data, idx.ctypes.data, 1, 1, ctypes.byref(h)) == _lib.ERR_HIP and h.value == 0
