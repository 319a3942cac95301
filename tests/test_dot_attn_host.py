"""CPU: scaled dot-product attention over the edges (gnnagg_dot_attn_run, Aggregator_GAT.run_dot, dot_attn_run) is declared, exported and
typed; every Python-side refusal raises before the library is reached; the float64 judge of tests/test_gpu_dot_attn.py -- a numpy
restatement of the formulas in include/gnnagg.h -- agrees with a 3-row example worked out by hand; and a sequential fp32 chain stays far
inside the bound the GPU tests hold the kernel to."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_gatv2_host import worst_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5   # the project's bar


# ------------------------------------------------------------------------------------------------------------------- the judge
def dot_attn_ref(ptr, idx, q, k, v, heads, scale, block_edges=1 << 15):
    """float64 dot-product attention over the CSR (ptr, idx): returns (y [V, F], L [V, heads], S [V, F]).
        e_j = scale * sum_c q[r, hD + c] k[j, hD + c];  alpha = softmax over the row's edges;  y[r] = sum_j alpha_j v[j]  (+0 for a row without
        edges);  L[r, h] = max_j |scale| sum_c |q k|;  S[r] = sum_j alpha_j |v[j]|.
    q / k / v are taken as given (float32 arrays: a bf16 input is judged on its exact widening); scale is the fp32 value the kernel gets."""
    ptr = np.asarray(ptr, np.int64)
    idx = np.asarray(idx, np.int64)
    V, F = len(ptr) - 1, q.shape[1]
    D = F // heads
    q64, k64, v64 = np.asarray(q, np.float64), np.asarray(k, np.float64), np.asarray(v, np.float64)
    sc = float(np.float32(scale))
    y, S, L = np.zeros((V, F)), np.zeros((V, F)), np.zeros((V, heads))
    r0 = 0
    while r0 < V:
        r1 = r0 + 1
        while r1 < V and ptr[r1 + 1] - ptr[r0] <= block_edges:
            r1 += 1
        e0, e1 = ptr[r0], ptr[r1]
        deg = np.diff(ptr[r0:r1 + 1])
        if e1 > e0:
            rows = np.repeat(np.arange(r0, r1), deg)
            src = v64[idx[e0:e1]]
            t = q64[rows] * k64[idx[e0:e1]]
            e = sc * t.reshape(-1, heads, D).sum(axis=2)
            labs = abs(sc) * np.abs(t).reshape(-1, heads, D).sum(axis=2)
            ne = np.flatnonzero(deg > 0)
            starts = (ptr[r0:r1][ne] - e0).astype(np.int64)
            mx = np.maximum.reduceat(e, starts, axis=0)
            local = np.repeat(np.arange(len(ne)), deg[ne])
            w = np.exp(e - mx[local])
            alpha = w / np.add.reduceat(w, starts, axis=0)[local]
            af = np.repeat(alpha, D, axis=1)
            y[r0 + ne] = np.add.reduceat(af * src, starts, axis=0)
            S[r0 + ne] = np.add.reduceat(af * np.abs(src), starts, axis=0)
            L[r0 + ne] = np.maximum.reduceat(labs, starts, axis=0)
        r0 = r1
    return y, L, S


def dot_attn_bound(L, S, heads):
    """the bound: 1e-5 * (1 + L[r, h]) * S[r, hD + c]"""
    return RTOL * (1.0 + np.repeat(L, S.shape[1] // heads, axis=1)) * S


def test_the_judge_agrees_with_a_hand_computed_example():
    # rows: 0 -> {1, 2}, 1 -> {}, 2 -> {0}; one head of two columns, scale 0.5 (exact in fp32)
    ptr, idx = np.array([0, 2, 2, 3]), np.array([1, 2, 0])
    q = np.array([[1, 2], [5, 5], [-1, 2]], np.float32)
    k = np.array([[1, 2], [3, -1], [0.5, 0]], np.float32)
    v = np.array([[1, -2], [3, -4], [0.5, 8]], np.float32)
    y, L, S = dot_attn_ref(ptr, idx, q, k, v, 1, 0.5)
    # row 0: e = 0.5 * (3 - 2) = 0.5 and 0.5 * (0.5 + 0) = 0.25;  softmax(0.5, 0.25)
    a1 = 1.0 / (1.0 + math.exp(-0.25))
    a2 = 1.0 - a1
    assert abs(a1 - 0.5621765008857981) < 1e-15
    np.testing.assert_allclose(y[0], [3 * a1 + 0.5 * a2, -4 * a1 + 8 * a2], rtol=1e-14)
    np.testing.assert_allclose(y[0], [1.9054412522144953, 1.2538819893704226], rtol=1e-12)
    np.testing.assert_allclose(S[0], [3 * a1 + 0.5 * a2, 4 * a1 + 8 * a2], rtol=1e-14)
    assert L[0, 0] == 2.5                  # max(0.5 * (|3| + |-2|), 0.5 * (0.5 + 0))
    # row 1: no edges -> +0, L = 0, S = 0
    assert np.all(y[1] == 0) and not np.signbit(y[1]).any() and L[1, 0] == 0 and np.all(S[1] == 0)
    # row 2: one edge -> its v row exactly; q k = (-1, 4) -> 0.5 * (1 + 4) = 2.5
    assert np.array_equal(y[2], [1.0, -2.0]) and L[2, 0] == 2.5 and np.array_equal(S[2], [1.0, 2.0])
    # two heads of one column each: every head is its own softmax.  head 0: e = 0.5 * (3, 0.5); head 1: e = 0.5 * (-2, 0)
    y2, L2, _ = dot_attn_ref(ptr, idx, q, k, v, 2, 0.5)
    b1 = 1.0 / (1.0 + math.exp(0.25 - 1.5))
    c1 = 1.0 / (1.0 + math.exp(0.0 - (-1.0)))
    np.testing.assert_allclose(y2[0], [3 * b1 + 0.5 * (1 - b1), -4 * c1 + 8 * (1 - c1)], rtol=1e-14)
    assert np.array_equal(L2[0], [1.5, 1.0]) and np.array_equal(L2[2], [0.5, 2.0])
    # a negative scale turns the order of the weights round, and L takes its magnitude
    y3, L3, _ = dot_attn_ref(ptr, idx, q, k, v, 1, -0.5)
    np.testing.assert_allclose(y3[0], [3 * a2 + 0.5 * a1, -4 * a2 + 8 * a1], rtol=1e-14)
    assert L3[0, 0] == 2.5
    # the bound and the ratio
    bound = dot_attn_bound(L, S, 1)
    np.testing.assert_allclose(bound[0], 1e-5 * 3.5 * S[0])
    assert worst_ratio(y, y, bound) == 0.0 and worst_ratio(y + bound, y, bound) == pytest.approx(1.0)
    off = y.copy()
    off[1, 0] = 1e-30
    assert worst_ratio(off, y, bound) == math.inf   # a row without edges has no slack


def test_the_judge_is_block_independent():
    rng = np.random.default_rng(0)
    ptr = np.concatenate([[0], np.cumsum(rng.integers(0, 9, 40))])
    idx = rng.integers(0, 60, ptr[-1])
    q, k, v = (rng.standard_normal((n, 12)).astype(np.float32) for n in (40, 60, 60))
    whole, small = dot_attn_ref(ptr, idx, q, k, v, 4, 0.3), dot_attn_ref(ptr, idx, q, k, v, 4, 0.3, block_edges=7)
    for a, b in zip(whole, small):
        assert np.array_equal(a, b)


def fp32_chain(ptr, idx, q, k, v, heads, scale):
    """the formulas as one sequential fp32 chain per element: the score column by column, then an online softmax that rescales at EVERY
    new maximum, edge by edge -- the longest chains and the most rescales any order of the kernel's can have"""
    f = np.float32
    V, F = len(ptr) - 1, q.shape[1]
    D = F // heads
    y = np.zeros((V, F), f)
    qs = (q * f(scale)).astype(f)
    for r in range(V):
        m, den, acc = np.full(heads, -np.inf, f), np.zeros(heads, f), np.zeros(F, f)
        for j in idx[ptr[r]:ptr[r + 1]]:
            e = np.zeros(heads, f)
            for c in range(D):
                e = (e + qs[r, c::D] * k[j, c::D]).astype(f)
            nm = np.maximum(m, e)
            with np.errstate(invalid="ignore"):
                sc = np.where(m == -np.inf, f(0), np.exp((m - nm).astype(f))).astype(f)
            w = np.exp((e - nm).astype(f)).astype(f)
            den = (den * sc + w).astype(f)
            acc = (acc * np.repeat(sc, D) + v[j] * np.repeat(w, D)).astype(f)
            m = nm
        if ptr[r + 1] > ptr[r]:
            y[r] = acc / np.repeat(den, D)
    return y


@pytest.mark.parametrize("H,D,mag,scale", [(1, 8, 1.0, None), (4, 3, 1.0, None), (2, 37, 1.0, None), (1, 8, 30.0, 1.0), (4, 3, 30.0, 1.0)])
def test_a_sequential_fp32_chain_stays_inside_the_bound(H, D, mag, scale):
    ptr, idx = gnc.graph.uniform_random_csr(60, 700, seed=5)
    ptr, idx = np.asarray(ptr), np.asarray(idx)
    V, F = len(ptr) - 1, H * D
    rng = np.random.default_rng(F)
    q, k, v = ((rng.standard_normal((V, F)) * mag).astype(np.float32) for _ in range(3))
    scale = np.float32(1.0 / math.sqrt(D)) if scale is None else np.float32(scale)
    ref, L, S = dot_attn_ref(ptr, idx, q, k, v, H, scale)
    ratio = worst_ratio(fp32_chain(ptr, idx, q, k, v, H, scale), ref, dot_attn_bound(L, S, H))
    print("fp32 chain %dx%d, inputs x%g, scale %g: worst ratio %.4f" % (H, D, mag, scale, ratio))
    assert ratio <= 1.0   # (seen here: a few hundredths -- the bound is reachable with room)


# ------------------------------------------------------------------------------------------------------- declared, exported, typed
def test_header_declares_and_the_library_exports_dot_attn():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    assert re.search(r"int gnnagg_dot_attn_run\(gnnagg_handle h, const void \*d_q, long long q_pitch, const void \*d_k, const void \*d_v, "
                     r"long long kv_pitch,\s+int x_dtype, void \*d_y, int y_dtype, int feat, int heads, float scale\);", text)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "gnnagg_dot_attn_run" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    res, args = _lib.SIGNATURES["gnnagg_dot_attn_run"]
    assert res is ctypes.c_int and args == [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float]
    assert gnc.lib().gnnagg_dot_attn_run.argtypes == args
    assert callable(gnc.dot_attn_run) and callable(gnc.Aggregator_GAT.run_dot)


def test_the_kernel_file_is_built_into_the_library():
    csrc = os.path.join(ROOT, "gnn_computing_amd", "csrc")
    kfiles = re.search(r"^KFILES := (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert "agg_dot" in kfiles and "agg_gatv2" in kfiles and os.path.exists(os.path.join(csrc, "agg_dot.hip"))


# --------------------------------------------------------------------------------------------------------------- Python-side refusals
class _NoDevice(Exception):
    pass


def _handleless_aggregator(monkeypatch, V=4):
    """an Aggregator_GAT without a device handle, whose every way into the library raises _NoDevice"""
    agg = gnc.Aggregator_GAT.__new__(gnc.Aggregator_GAT)
    agg.num_v, agg.num_e, agg.feat_in, agg.feat_out, agg._h = V, 0, 8, 8, ctypes.c_int64(0)

    def no_device():
        raise _NoDevice()
    monkeypatch.setattr(gnc.aggregator, "lib", no_device)
    monkeypatch.setattr(gnc.aggregator.Aggregator, "_use_current_stream", lambda self: no_device())
    return agg


def test_run_dot_refuses_before_the_library_is_reached(monkeypatch):
    agg = _handleless_aggregator(monkeypatch)
    f32, b16 = torch.zeros((4, 8)), torch.zeros((4, 8), dtype=torch.bfloat16)
    for run in (lambda *p, **kw: agg.run_dot(*p, **kw), lambda *p, **kw: gnc.dot_attn_run(agg, *p, **kw)):
        for other in (torch.zeros((4, 8), dtype=torch.float16), torch.zeros((4, 8), dtype=torch.float64), np.zeros((4, 8), np.float32)):
            for pos in range(4):
                ops = [f32, f32, f32, f32]
                ops[pos] = other
                with pytest.raises(TypeError):
                    run(*ops, heads=2)
        for ops in ((f32, b16, f32, f32), (f32, f32, b16, f32), (b16, f32, f32, b16), (b16, b16, f32, f32)):
            with pytest.raises(TypeError, match="q's dtype"):
                run(*ops, heads=2)
        # stride(1) != 1
        wide = torch.zeros((4, 16))
        for pos in range(3):
            ops = [f32, f32, f32, f32]
            ops[pos] = wide[:, ::2]
            with pytest.raises(ValueError, match=r"stride\(1\)"):
                run(*ops, heads=2)
        with pytest.raises(ValueError, match=r"stride\(1\)"):
            run(torch.zeros((8, 4)).t(), f32, f32, f32, heads=2)
        # k and v: one pitch, one shape
        with pytest.raises(ValueError, match="one row pitch"):
            run(f32, wide[:, :8], f32, f32, heads=2)
        with pytest.raises(ValueError, match="one shape"):
            run(f32, torch.zeros((5, 8)), f32, f32, heads=2)
        with pytest.raises(ValueError, match="columns"):
            run(f32, torch.zeros((4, 6)), torch.zeros((4, 6)), f32, heads=2)
        with pytest.raises(ValueError, match="does not divide"):
            run(f32, f32, f32, f32, heads=3)
        with pytest.raises(ValueError, match="does not divide"):
            run(f32, f32, f32, f32, heads=0)
        with pytest.raises(ValueError, match=r"must be \[rows, F\]"):
            run(torch.zeros(32), f32, f32, f32, heads=2)
        with pytest.raises(ValueError, match="q must hold"):
            run(torch.zeros((3, 8)), f32, f32, f32, heads=2)
        with pytest.raises(ValueError, match="vout must hold"):
            run(f32, f32, f32, torch.zeros((3, 8)), heads=2)
        with pytest.raises(ValueError, match="row pitch"):
            run(f32, f32.as_strided((4, 8), (4, 1)), f32.as_strided((4, 8), (4, 1)), f32, heads=2)
        for bad in (float("nan"), float("inf"), -float("inf"), 1e39):
            with pytest.raises(ValueError, match="not finite"):
                run(f32, f32, f32, f32, heads=2, scale=bad)
        # what passes the checks reaches the library (here: the stub): all four dtype pairs, one tensor for the three operands, more source
        # rows than V, either sign of the scale, and the column views of one packed [n, 3F] tensor
        for x, y in ((f32, f32), (f32, b16), (b16, f32), (b16, b16)):
            with pytest.raises(_NoDevice):
                run(x, x, x, y, heads=2)
            big = torch.zeros((9, 8), dtype=x.dtype)
            with pytest.raises(_NoDevice):
                run(x, big, big.clone(), y, heads=2, scale=-0.5)
            qkv = torch.zeros((9, 24), dtype=x.dtype)
            with pytest.raises(_NoDevice):
                run(qkv[:, :8], qkv[:, 8:16], qkv[:, 16:], y, heads=4, scale=0.0)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_the_call_errors_out_without_a_gpu():
    L = gnc.lib()
    x, y = np.zeros(8, np.float32), np.zeros(8, np.float32)
    rc = L.gnnagg_dot_attn_run(ctypes.c_int64(0), x.ctypes.data, 8, x.ctypes.data, x.ctypes.data, 8, 0, y.ctypes.data, 0, 8, 1, ctypes.c_float(0.5))
    assert rc == _lib.ERR_ARG and b"handle" in L.gnnagg_last_error()
