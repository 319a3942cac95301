"""CPU: GATv2 attention (gnnagg_gatv2_run, Aggregator_GAT.run_v2, gatv2_run) is declared, exported and typed; every Python-side refusal
raises before the library is reached; and the float64 judge of tests/test_gpu_gatv2.py -- a numpy restatement of the formulas in
include/gnnagg.h -- agrees with a 3-row example worked out by hand."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5   # the project's bar


# ------------------------------------------------------------------------------------------------------------------- the judge
def gatv2_ref(ptr, idx, xs, xd, a, heads, slope=0.2, block_edges=1 << 15):
    """float64 GATv2 over the CSR (ptr, idx): returns (y [V, F], L [V, heads], S [V, F]).
        z = xd[r] + xs[j];  l = z > z * slope ? z : z * slope;  e_j = sum_c a[h, c] l_jc;  alpha = softmax over the row's edges;
        y[r] = sum_j alpha_j xs[j]  (+0 for a row without edges);  L[r, h] = max_j sum_c |a[h, c] l_jc|;  S[r] = sum_j alpha_j |xs[j]|.
    xs / xd / a are taken as given (float32 arrays: a bf16 input is judged on its exact widening); slope is the fp32 value the kernel gets."""
    ptr = np.asarray(ptr, np.int64)
    idx = np.asarray(idx, np.int64)
    V, F = len(ptr) - 1, xs.shape[1]
    D = F // heads
    xs64, xd64 = np.asarray(xs, np.float64), np.asarray(xd, np.float64)
    a64 = np.asarray(a, np.float64).reshape(1, F)
    sl = float(np.float32(slope))
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
            src = xs64[idx[e0:e1]]
            z = xd64[rows] + src
            zs = z * sl
            t = a64 * np.where(z > zs, z, zs)
            e = t.reshape(-1, heads, D).sum(axis=2)
            labs = np.abs(t).reshape(-1, heads, D).sum(axis=2)
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


def gatv2_bound(L, S, heads):
    """the issue's bound: 1e-5 * (1 + L[r, h]) * S[r, hD + c]"""
    return RTOL * (1.0 + np.repeat(L, S.shape[1] // heads, axis=1)) * S


def worst_ratio(y, ref, bound):
    """max |y - ref| / bound over the whole output; 0 / 0 (rows without edges: y must be exactly 0) counts as 0, x / 0 as inf"""
    err = np.abs(np.asarray(y, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def test_the_judge_agrees_with_a_hand_computed_example():
    # rows: 0 -> {1, 2}, 1 -> {}, 2 -> {0}; one head of two columns, slope 0.5 (exact in fp32)
    ptr, idx = np.array([0, 2, 2, 3]), np.array([1, 2, 0])
    xs = np.array([[1, 2], [3, -4], [0.5, 0]], np.float32)
    xd = np.array([[0, 0], [1, 1], [-1, 2]], np.float32)
    a = np.array([[1, 0.5]], np.float32)
    y, L, S = gatv2_ref(ptr, idx, xs, xd, a, 1, slope=0.5)
    # row 0: z = (3, -4) -> l = (3, -2) -> e = 3 - 1 = 2;  z = (0.5, 0) -> l = (0.5, 0) -> e = 0.5;  softmax(2, 0.5)
    a1 = 1.0 / (1.0 + math.exp(-1.5))
    a2 = 1.0 - a1
    assert abs(a1 - 0.8175744761936437) < 1e-15
    np.testing.assert_allclose(y[0], [3 * a1 + 0.5 * a2, -4 * a1], rtol=1e-14)
    np.testing.assert_allclose(y[0], [2.5439361904841093, -3.270297904774575], rtol=1e-12)
    np.testing.assert_allclose(S[0], [2.5439361904841093, 3.270297904774575], rtol=1e-12)
    assert L[0, 0] == 4.0                  # max(|3| + |0.5 * -2|, |0.5| + 0)
    # row 1: no edges -> +0, L = 0, S = 0
    assert np.all(y[1] == 0) and not np.signbit(y[1]).any() and L[1, 0] == 0 and np.all(S[1] == 0)
    # row 2: one edge -> its source row exactly; z = (0, 4) -> sum |a l| = 2
    assert np.array_equal(y[2], [1.0, 2.0]) and L[2, 0] == 2.0 and np.array_equal(S[2], [1.0, 2.0])
    # two heads of one column each: every head is its own softmax
    y2, L2, _ = gatv2_ref(ptr, idx, xs, xd, np.array([[1], [0.5]], np.float32), 2, slope=0.5)
    b1 = 1.0 / (1.0 + math.exp(0.5 - 3.0))          # head 0: e = (3, 0.5)
    c1 = 1.0 / (1.0 + math.exp(0.0 - (-1.0)))       # head 1: e = (0.5 * -2, 0) = (-1, 0)
    np.testing.assert_allclose(y2[0], [3 * b1 + 0.5 * (1 - b1), -4 * c1], rtol=1e-14)
    assert np.array_equal(L2[0], [3.0, 1.0])
    # the bound and the ratio
    bound = gatv2_bound(L, S, 1)
    np.testing.assert_allclose(bound[0], 1e-5 * 5.0 * S[0])
    assert worst_ratio(y, y, bound) == 0.0 and worst_ratio(y + bound, y, bound) == pytest.approx(1.0)
    off = y.copy()
    off[1, 0] = 1e-30
    assert worst_ratio(off, y, bound) == math.inf   # a row without edges has no slack


def test_the_judge_is_block_independent():
    rng = np.random.default_rng(0)
    ptr = np.concatenate([[0], np.cumsum(rng.integers(0, 9, 40))])
    idx = rng.integers(0, 60, ptr[-1])
    xs, xd, a = rng.standard_normal((60, 12)).astype(np.float32), rng.standard_normal((40, 12)).astype(np.float32), rng.standard_normal((4, 3)).astype(np.float32)
    whole, small = gatv2_ref(ptr, idx, xs, xd, a, 4), gatv2_ref(ptr, idx, xs, xd, a, 4, block_edges=7)
    for u, v in zip(whole, small):
        assert np.array_equal(u, v)


# ------------------------------------------------------------------------------------------------------- declared, exported, typed
def test_header_declares_and_the_library_exports_gatv2():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    assert re.search(r"int gnnagg_gatv2_run\(gnnagg_handle h, const void \*d_xs, const void \*d_xd, int x_dtype, const float \*d_a, void \*d_y, "
                     r"int y_dtype, int feat,\s+int heads, float slope\);", text)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "gnnagg_gatv2_run" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    res, args = _lib.SIGNATURES["gnnagg_gatv2_run"]
    assert res is ctypes.c_int and args == [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float]
    assert gnc.lib().gnnagg_gatv2_run.argtypes == args
    assert callable(gnc.gatv2_run) and callable(gnc.Aggregator_GAT.run_v2)


def test_thresholds_mirror_common_h():
    text = open(os.path.join(ROOT, "gnn_computing_amd", "csrc", "common.h")).read()
    m = re.search(r"constexpr int kGatv2Batch = (\d+), kGatv2LongEdges = (\d+), kGatv2SegEdges = (\d+), kGatv2MaxFeat = (\d+);", text)
    batch, long_edges, seg_edges, max_feat = (int(g) for g in m.groups())
    assert gnc.Aggregator_GAT.GATV2_THRESHOLDS == (batch, 8, 16, 32, 64, long_edges, seg_edges)
    assert gnc.Aggregator_GAT.GATV2_MAX_FEAT == max_feat
    assert "feat > %d (the kernel's limit)" % max_feat in open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    kfiles = re.search(r"^KFILES := (.*)$", open(os.path.join(ROOT, "gnn_computing_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "agg_gatv2" in kfiles and os.path.exists(os.path.join(ROOT, "gnn_computing_amd", "csrc", "agg_gatv2.hip"))


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


def test_run_v2_refuses_before_the_library_is_reached(monkeypatch):
    agg = _handleless_aggregator(monkeypatch)
    f32, b16 = torch.zeros((4, 8)), torch.zeros((4, 8), dtype=torch.bfloat16)
    a = torch.zeros((2, 4))
    for run in (lambda *p, **k: agg.run_v2(*p, **k), lambda *p, **k: gnc.gatv2_run(agg, *p, **k)):
        for other in (torch.zeros((4, 8), dtype=torch.float16), torch.zeros((4, 8), dtype=torch.float64), np.zeros((4, 8), np.float32)):
            with pytest.raises(TypeError):
                run(other, f32, a, f32, heads=2)
            with pytest.raises(TypeError):
                run(f32, other, a, f32, heads=2)
            with pytest.raises(TypeError):
                run(f32, f32, a, other, heads=2)
        with pytest.raises(TypeError, match="xs's dtype"):
            run(f32, b16, a, f32, heads=2)
        with pytest.raises(TypeError, match="xs's dtype"):
            run(b16, f32, a, b16, heads=2)
        with pytest.raises(TypeError, match="a must be"):
            run(f32, f32, a.to(torch.bfloat16), f32, heads=2)
        with pytest.raises(TypeError, match="a must be"):
            run(b16, b16, a.numpy(), f32, heads=2)
        with pytest.raises(ValueError, match="does not divide"):
            run(f32, f32, a, f32, heads=3)
        with pytest.raises(ValueError, match="does not divide"):
            run(f32, f32, a, f32, heads=0)
        with pytest.raises(ValueError, match="does not hold"):
            run(f32, f32, torch.zeros((2, 3)), f32, heads=2)
        with pytest.raises(ValueError, match="xs must be"):
            run(torch.zeros(32), f32, a, f32, heads=2)
        with pytest.raises(ValueError, match="xd must hold"):
            run(f32, torch.zeros((3, 8)), a, f32, heads=2)
        with pytest.raises(ValueError, match="vout must hold"):
            run(f32, f32, a, torch.zeros((3, 8)), heads=2)
        # what passes the checks reaches the library (here: the stub), in all four dtype pairs and with xd is xs
        for x, y in ((f32, f32), (f32, b16), (b16, f32), (b16, b16)):
            with pytest.raises(_NoDevice):
                run(x, x, a, y, heads=2)
            with pytest.raises(_NoDevice):
                run(torch.zeros((9, 8), dtype=x.dtype), x, a, y, heads=2)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_the_call_errors_out_without_a_gpu():
    L = gnc.lib()
    x, a, y = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.float32)
    rc = L.gnnagg_gatv2_run(ctypes.c_int64(0), x.ctypes.data, x.ctypes.data, 0, a.ctypes.data, y.ctypes.data, 0, 8, 1, ctypes.c_float(0.2))
    assert rc == _lib.ERR_ARG and b"handle" in L.gnnagg_last_error()
