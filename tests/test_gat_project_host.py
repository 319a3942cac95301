"""CPU: gnnagg_gat_project (the GAT projection and its attention terms in one call) is declared, exported and typed; it refuses every dtype
combination but fp32.fp32->fp32 and bf16.bf16->fp32/bf16, bad head counts, negative sizes and NULL operands before any device call;
gnc.gat_project checks devices, dtypes and shapes before it reaches the library."""
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
F32, BF16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
ACCEPTED = [(F32, F32, F32), (BF16, BF16, F32), (BF16, BF16, BF16)]


def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    assert re.search(r"int gnnagg_gat_project\(const void \*d_x, int x_dtype, const void \*d_w, int w_dtype,\s+"
                     r"const void \*d_a_dst, const void \*d_a_src,[^\n]*\n\s+void \*d_feat, int feat_dtype, float \*d_att,[^\n]*\n\s+"
                     r"int m, int n, int k, int heads, int \*path, void \*hip_stream\);", text)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "gnnagg_gat_project" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    res, args = _lib.SIGNATURES["gnnagg_gat_project"]
    c_int, c_void_p = ctypes.c_int, ctypes.c_void_p
    assert res is c_int and args == [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                     ctypes.POINTER(c_int), c_void_p]
    assert gnc.lib().gnnagg_gat_project.argtypes == args


def _call(tx, tw, tf, m=4, n=4, k=4, heads=1, null=None):
    """the call on dummy host pointers: only argument checks may run"""
    L = gnc.lib()
    buf = np.zeros(64, np.float32)
    p = {name: buf.ctypes.data for name in ("x", "w", "a_dst", "a_src", "feat", "att")}
    if null:
        p[null] = None
    path = ctypes.c_int(-1)
    rc = L.gnnagg_gat_project(p["x"], tx, p["w"], tw, p["a_dst"], p["a_src"], p["feat"], tf, p["att"], m, n, k, heads, ctypes.byref(path), None)
    return rc, L.gnnagg_last_error().decode()


@pytest.mark.parametrize("combo,names", [((7, 0, 0), ("7",)), ((0, 0, 2), ("2",)), ((0, -1, 0), ("-1",)),
                                         ((BF16, F32, F32), ("x bf16", "w fp32", "feat fp32")),
                                         ((F32, BF16, F32), ("x fp32", "w bf16", "feat fp32")),
                                         ((F32, BF16, BF16), ("x fp32", "w bf16", "feat bf16")),
                                         ((BF16, F32, BF16), ("x bf16", "w fp32", "feat bf16")),
                                         ((F32, F32, BF16), ("x fp32", "w fp32", "feat bf16"))])
def test_other_dtype_combinations_are_refused_by_name_without_a_device(combo, names):
    rc, msg = _call(*combo)
    assert rc == _lib.ERR_ARG and "gnnagg_gat_project" in msg
    for nm in names:
        assert nm in msg, msg


@pytest.mark.parametrize("combo", ACCEPTED)
def test_sizes_heads_and_null_operands_are_checked_before_any_device_call(combo):
    for kw in (dict(m=-1), dict(n=-4), dict(k=-1), dict(heads=0), dict(heads=-2), dict(n=6, heads=4), dict(n=4, heads=8)):
        rc, msg = _call(*combo, **kw)
        assert rc == _lib.ERR_ARG and "gnnagg_gat_project" in msg, (kw, msg)
    for name in ("x", "w", "a_dst", "a_src", "feat", "att"):
        rc, msg = _call(*combo, null=name)
        assert rc == _lib.ERR_ARG and "gnnagg_gat_project" in msg, (name, msg)
    assert _call(*combo, m=0)[0] == _lib.OK      # nothing to do: no device is touched (this machine may have none)
    assert _call(*combo, m=0, null="x")[0] == _lib.OK


class _NoDevice(Exception):
    pass


@pytest.fixture
def stub(monkeypatch):
    def no_device():
        raise _NoDevice()
    monkeypatch.setattr(gnc.aggregator, "lib", no_device)


def _operands(dtype=torch.float32, M=4, K=8, N=6, heads=2):
    return (torch.zeros((M, K), dtype=dtype), torch.zeros((K, N), dtype=dtype), torch.zeros((heads, N // heads), dtype=dtype),
            torch.zeros((heads, N // heads), dtype=dtype))


def test_gat_project_refuses_host_tensors_before_the_library(stub):
    for dtype in (torch.float32, torch.bfloat16):
        x, W, ad, as_ = _operands(dtype)
        with pytest.raises(ValueError, match="device tensor"):
            gnc.gat_project(x, W, ad, as_, heads=2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_gat_project_rejects_other_dtypes_before_the_library(stub, dtype):
    x, W, ad, as_ = _operands()
    xb, Wb, adb, asb = _operands(torch.bfloat16)
    o = lambda t: t.to(dtype)
    for args, kw in (((o(x), W, ad, as_), {}), ((x, o(W), ad, as_), {}), ((x, W, o(ad), as_), {}), ((x, W, ad, o(as_)), {}),
                     ((xb, W, ad, as_), {}), ((x, Wb, adb, asb), {}), ((xb, Wb, ad, asb), {}), ((xb, Wb, adb, as_), {}),
                     ((x, W, ad, as_), dict(out_dtype=dtype)), ((x, W, ad, as_), dict(out_dtype=torch.bfloat16)),
                     ((x, W, ad, as_), dict(feat=torch.zeros((4, 6), dtype=torch.bfloat16))),
                     ((xb, Wb, adb, asb), dict(feat=torch.zeros((4, 6), dtype=dtype))),
                     ((xb, Wb, adb, asb), dict(feat=torch.zeros((4, 6)), out_dtype=torch.bfloat16)),
                     ((xb, Wb, adb, asb), dict(att=torch.zeros((4, 2, 2), dtype=torch.bfloat16)))):
        with pytest.raises(TypeError):
            gnc.gat_project(*args, heads=2, **kw)


def test_gat_project_rejects_mismatched_shapes_before_the_library(stub):
    x, W, ad, as_ = _operands()
    for args, kw in (((torch.zeros((4, 7)), W, ad, as_), dict(heads=2)),            # x and W do not multiply
                     ((x, W, ad, as_), dict(heads=4)),                              # heads does not divide N
                     ((x, W, ad, as_), dict(heads=0)),
                     ((x, W, torch.zeros((3, 2)), as_), dict(heads=2)),             # a_dst is not [heads, D]
                     ((x, W, ad, torch.zeros((2, 4))), dict(heads=2)),
                     ((x, W, torch.zeros(5), torch.zeros(5)), dict(heads=1)),       # heads = 1: N elements
                     ((x, W, ad, as_), dict(heads=2, feat=torch.zeros((4, 5)))),
                     ((x, W, ad, as_), dict(heads=2, att=torch.zeros((4, 2, 3)))),
                     ((x[0], W, ad, as_), dict(heads=2))):
        with pytest.raises(ValueError):
            gnc.gat_project(*args, **kw)


def test_last_project_path_is_exported():
    assert gnc.last_project_path() in (0, 1, 2)
