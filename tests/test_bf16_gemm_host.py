"""CPU: the typed dense combine (gnnagg_matmul_nn_typed) is declared, exported and typed; it refuses every dtype combination but
fp32.fp32->fp32 and bf16.bf16->fp32/bf16 before any device call; gnc.matmul_NN checks dtypes and shapes before it reaches the library."""
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


def test_header_declares_and_library_exports_the_typed_entry_point():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    assert re.search(r"int gnnagg_matmul_nn_typed\(const void \*d_a, int a_dtype, const void \*d_b, int b_dtype, void \*d_c, int c_dtype,\s+"
                     r"int m, int n, int k, void \*hip_stream\);", text)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "gnnagg_matmul_nn_typed" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    res, args = _lib.SIGNATURES["gnnagg_matmul_nn_typed"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert gnc.lib().gnnagg_matmul_nn_typed.argtypes == args


def _call(ta, tb, tc, m=4, n=4, k=4):
    """the typed call on dummy host pointers: only argument checks may run"""
    L = gnc.lib()
    buf = np.zeros(64, np.float32)
    rc = L.gnnagg_matmul_nn_typed(buf.ctypes.data, ta, buf.ctypes.data, tb, buf.ctypes.data, tc, m, n, k, None)
    return rc, L.gnnagg_last_error().decode()


@pytest.mark.parametrize("combo,names", [((7, 0, 0), ("7",)), ((BF16, F32, F32), ("a bf16", "b fp32", "c fp32")),
                                         ((F32, BF16, F32), ("a fp32", "b bf16", "c fp32")),
                                         ((F32, F32, BF16), ("a fp32", "b fp32", "c bf16"))])
def test_other_dtype_combinations_are_refused_by_name_without_a_device(combo, names):
    rc, msg = _call(*combo)
    assert rc == _lib.ERR_ARG and "gnnagg_matmul_nn_typed" in msg
    for nm in names:
        assert nm in msg, msg


@pytest.mark.parametrize("combo", [(F32, F32, F32), (BF16, BF16, F32), (BF16, BF16, BF16)])
def test_sizes_are_checked_before_any_device_call(combo):
    assert _call(*combo, m=-1)[0] == _lib.ERR_ARG
    assert _call(*combo, k=-1)[0] == _lib.ERR_ARG
    L = gnc.lib()
    assert L.gnnagg_matmul_nn_typed(None, combo[0], None, combo[1], None, combo[2], 4, 4, 4, None) == _lib.ERR_ARG   # NULL operands
    assert _call(*combo, m=0)[0] == _lib.OK      # nothing to do: no device is touched (this machine may have none)
    assert _call(*combo, n=0)[0] == _lib.OK


class _NoDevice(Exception):
    pass


@pytest.fixture
def stub(monkeypatch):
    def no_device():
        raise _NoDevice()
    monkeypatch.setattr(gnc.aggregator, "lib", no_device)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_matmul_NN_rejects_other_dtypes_before_the_library(stub, dtype):
    f32, b16, other = torch.zeros((4, 8)), torch.zeros((4, 8), dtype=torch.bfloat16), torch.zeros((4, 8), dtype=dtype)
    w32, w16, wo = torch.zeros((8, 3)), torch.zeros((8, 3), dtype=torch.bfloat16), torch.zeros((8, 3), dtype=dtype)
    co = torch.zeros((4, 3), dtype=dtype)
    for a, b, c in ((other, w32, None), (f32, wo, None), (other, w16, None), (b16, wo, None), (b16, w16, co), (f32, w32, co)):
        with pytest.raises(TypeError, match="float32 or torch.bfloat16"):
            gnc.matmul_NN(a, b, c)
    with pytest.raises(TypeError):
        gnc.matmul_NN(b16, w16, out_dtype=dtype)


def test_matmul_NN_reaches_the_library_with_bf16_and_fp32(stub):
    f32, b16 = torch.zeros((4, 8)), torch.zeros((4, 8), dtype=torch.bfloat16)
    w32, w16 = torch.zeros((8, 3)), torch.zeros((8, 3), dtype=torch.bfloat16)
    for a, b, kw in ((b16, w16, {}), (b16, w16, dict(out_dtype=torch.float32)), (b16, w16, dict(C=torch.zeros((4, 3)))),
                     (b16, w16, dict(C=torch.zeros((4, 3), dtype=torch.bfloat16))), (f32, w32, {})):
        with pytest.raises(_NoDevice):
            gnc.matmul_NN(a, b, **kw)


def test_matmul_NN_rejects_mismatched_shapes(stub):
    b16 = torch.zeros((4, 8), dtype=torch.bfloat16)
    for a, b, c in ((b16, torch.zeros((7, 3), dtype=torch.bfloat16), None),
                    (b16, torch.zeros((8, 3), dtype=torch.bfloat16), torch.zeros((4, 4))),
                    (b16, torch.zeros((8, 3), dtype=torch.bfloat16), torch.zeros((5, 3), dtype=torch.bfloat16)),
                    (torch.zeros((4, 8)), torch.zeros((9, 3)), None)):
        with pytest.raises(ValueError):
            gnc.matmul_NN(a, b, c)
