"""Host: the per-edge score bias of the two online-softmax attention calls (gnnagg_gatv2_run_bias / Aggregator_GAT.run_v2(bias=),
gnnagg_dot_attn_run_bias / Aggregator_GAT.run_dot(bias=)) -- the judges, inputs and expectations of tests/test_gpu_attn_bias.py, pinned
without a GPU.

  * dot_attn_bias_ref / gatv2_bias_ref: the float64 two-pass formulas of include/gnnagg.h with the bias added to the score.  They return
    (y, L, S) with L[r, h] = max over the row's edges with a FINITE bias of (the unbiased call's L term + |bias|): the bias is one more
    term of the score, so it widens the score's condition number by its magnitude; a masked edge (-Inf) has no weight and no part in L.
  * the bound 1e-5 (1 + L) S with that L, and a sequential fp32 chain (score chain, ONE fp32 add of the bias, two-pass softmax in fp32)
    that stays inside it on the GPU file's inputs;
  * the spread condition of the class maps (finite float64 scores of a (row, head) within 60 of each other) on those inputs;
  * the declarations, the Python-side refusals and the entry point each call reaches;
  * the fp32 emulation of the kernels' recurrence (tests/test_attn_nonfinite_host.py) with -Inf scores made by a bias."""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_attn_nonfinite_host import (NINF, PATTERNS, ROW_LENGTHS, SCORED, SHAPES, SLOPE, SPREAD, attn_operands, bf16_exact, check_row,
                                      default_scale, delete_edges, emulate_row, full_ref, head_scores, mask_edges, one_row, pattern_id,
                                      reserve_sources, row_judge, small_graph)
from test_dot_attn_host import _NoDevice, dot_attn_bound, dot_attn_ref
from test_gatv2_host import gatv2_bound, gatv2_ref, worst_ratio
from test_gpu_gatv2 import threshold_graph
from test_nonfinite_host import classes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------- the judges
def _bias_ref(ptr, idx, term, src, heads, bias, block_edges):
    """the two-pass float64 softmax and sum over the CSR with scores mult * sum_c t + bias; term(rows, cols) -> (t [n, F], mult)"""
    ptr = np.asarray(ptr, np.int64)
    idx = np.asarray(idx, np.int64)
    V, F = len(ptr) - 1, src.shape[1]
    D = F // heads
    src64 = np.asarray(src, np.float64)
    b64 = np.asarray(bias, np.float64)
    b64 = b64.reshape(len(idx), b64.shape[1] if b64.ndim == 2 else 1)      # (a graph without edges has a bias without elements)
    assert b64.shape[1] in (1, heads)
    y, S, L = np.zeros((V, F)), np.zeros((V, F)), np.zeros((V, heads))
    r0 = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while r0 < V:
            r1 = r0 + 1
            while r1 < V and ptr[r1 + 1] - ptr[r0] <= block_edges:
                r1 += 1
            e0, e1 = ptr[r0], ptr[r1]
            deg = np.diff(ptr[r0:r1 + 1])
            if e1 > e0:
                rows = np.repeat(np.arange(r0, r1), deg)
                s = src64[idx[e0:e1]]
                t, mult = term(rows, idx[e0:e1])
                b = np.broadcast_to(b64[e0:e1], (e1 - e0, heads))
                e = mult * t.reshape(-1, heads, D).sum(axis=2) + b
                labs = np.where(np.isfinite(b), abs(mult) * np.abs(t).reshape(-1, heads, D).sum(axis=2) + np.abs(b), 0.0)
                ne = np.flatnonzero(deg > 0)
                starts = (ptr[r0:r1][ne] - e0).astype(np.int64)
                mx = np.maximum.reduceat(e, starts, axis=0)
                local = np.repeat(np.arange(len(ne)), deg[ne])
                w = np.exp(e - mx[local])
                alpha = w / np.add.reduceat(w, starts, axis=0)[local]
                af = np.repeat(alpha, D, axis=1)
                y[r0 + ne] = np.add.reduceat(af * s, starts, axis=0)
                S[r0 + ne] = np.add.reduceat(af * np.abs(s), starts, axis=0)
                L[r0 + ne] = np.maximum.reduceat(labs, starts, axis=0)
            r0 = r1
    return y, L, S


def dot_attn_bias_ref(ptr, idx, q, k, v, heads, scale, bias, block_edges=1 << 15):
    """dot_attn_ref (tests/test_dot_attn_host.py) with e_p = scale * sum_c q k + bias[p, h]; bias [E], [E, 1] or [E, heads].
    L[r, h] = max over the row's edges with a finite bias of (|scale| sum_c |q k| + |bias|) (0 where there is none)."""
    q64, k64 = np.asarray(q, np.float64), np.asarray(k, np.float64)
    return _bias_ref(ptr, idx, lambda rows, cols: (q64[rows] * k64[cols], float(np.float32(scale))), v, heads, bias, block_edges)


def gatv2_bias_ref(ptr, idx, xs, xd, a, heads, slope, bias, block_edges=1 << 15):
    """gatv2_ref (tests/test_gatv2_host.py) with e_p = sum_c a l + bias[p, h]; L[r, h] = max over finite-bias edges of (sum_c |a l| + |bias|)"""
    xs64, xd64 = np.asarray(xs, np.float64), np.asarray(xd, np.float64)
    a64 = np.asarray(a, np.float64).reshape(1, xs.shape[1])
    sl = float(np.float32(slope))

    def term(rows, cols):
        z = xd64[rows] + xs64[cols]
        zs = z * sl
        return a64 * np.where(z > zs, z, zs), 1.0
    return _bias_ref(ptr, idx, term, xs, heads, bias, block_edges)


def bias_ref(call, ptr, idx, ops, H, bias, block_edges=1024):
    """the judge of one call on the operands of attn_operands (default scale, slope 0.2): (y, L, S)"""
    D = ops[SCORED[call]].shape[1] // H
    if call == "dot":
        return dot_attn_bias_ref(ptr, idx, ops["q"], ops["k"], ops["v"], H, default_scale(D), bias, block_edges)
    return gatv2_bias_ref(ptr, idx, ops["xs"], ops["xd"], ops["a"], H, SLOPE, bias, block_edges)


def bias_bound(L, S, heads):
    """the project's bound with the widened L: 1e-5 * (1 + L[r, h]) * S[r, hD + c]"""
    return dot_attn_bound(L, S, heads)


def test_the_bound_is_the_projects_own():
    L, S = np.array([[1.0, 3.0]]), np.array([[1.0, 2.0, 3.0, 4.0]])
    assert np.array_equal(bias_bound(L, S, 2), gatv2_bound(L, S, 2)) and np.allclose(bias_bound(L, S, 2), 1e-5 * np.array([[2, 4, 12, 16]]))


# ------------------------------------------------------------------------------------------------------------------- the inputs
PTR, IDX0, N_SRC = threshold_graph(n_src_extra=300)
IDX = reserve_sources(IDX0, N_SRC)[0]       # the ids of tests/test_gpu_attn_nonfinite.py's clean runs
V, E = len(PTR) - 1, len(IDX0)
DEG = np.diff(PTR)


def head_of(H):
    return H // 2


def case_operands(call, H, D):
    """the operands of the GPU file's cases on the threshold graph (bf16-exact; shared, read-only)"""
    return attn_operands(call, V, N_SRC, H, D, head_of(H), seed=H * D)


@functools.lru_cache(maxsize=None)
def _random_bias(n_e, cols, seed):
    b = bf16_exact(2.0 * np.random.default_rng(seed).standard_normal((n_e, cols), dtype=np.float32))
    b.setflags(write=False)
    return b


def random_bias(H, per_head, n_e=E):
    """bf16-exact 2 * randn: [E, H], or [E] (one value per edge for every head); read-only"""
    b = _random_bias(n_e, H if per_head else 1, 7000 + H)
    return b if per_head else b.reshape(n_e)


def test_zero_bias_is_the_unbiased_judge_exactly():
    ptr, idx, n_src = small_graph()
    n_v = len(ptr) - 1
    for H, D in ((3, 4), (1, 8)):
        for call in ("dot", "v2"):
            ops = attn_operands(call, n_v, n_src, H, D, 0, seed=40)
            want = full_ref(call, ptr, idx, ops, H)
            for zero in (np.zeros(len(idx), f32), np.zeros((len(idx), 1), f32), np.zeros((len(idx), H), f32)):
                got = bias_ref(call, ptr, idx, ops, H, zero)
                for a, b in zip(got, want):
                    assert np.array_equal(a, b)


def test_the_judges_agree_with_a_hand_computed_example():
    # rows: 0 -> {1, 2, 0}, 1 -> {}, 2 -> {0}; the third edge of row 0 is masked
    ptr, idx = np.array([0, 3, 3, 4]), np.array([1, 2, 0, 0])
    inf = np.inf
    # ---- dot-product: q, k, v and scale 0.5 of tests/test_dot_attn_host.py; unbiased scores of row 0: 0.5, 0.25 (and 2.5 for the masked edge)
    q = np.array([[1, 2], [5, 5], [-1, 2]], f32)
    k = np.array([[1, 2], [3, -1], [0.5, 0]], f32)
    v = np.array([[1, -2], [3, -4], [0.5, 8]], f32)
    for bias in (np.array([0.25, -0.5, -inf, 3.0], f32), np.array([[0.25], [-0.5], [-inf], [3.0]], f32)):     # bias_heads = 1
        y, L, S = dot_attn_bias_ref(ptr, idx, q, k, v, 1, 0.5, bias)
        a1 = 1.0 / (1.0 + math.exp(-0.25 - 0.75))      # e = 0.75 and -0.25
        a2 = 1.0 - a1
        np.testing.assert_allclose(y[0], [3 * a1 + 0.5 * a2, -4 * a1 + 8 * a2], rtol=1e-14)
        np.testing.assert_allclose(S[0], [3 * a1 + 0.5 * a2, 4 * a1 + 8 * a2], rtol=1e-14)
        assert L[0, 0] == 2.75                        # max(2.5 + 0.25, 0.25 + 0.5); the masked edge (2.5 + inf) has no part
        assert np.all(y[1] == 0) and not np.signbit(y[1]).any() and L[1, 0] == 0 and np.all(S[1] == 0)
        assert np.array_equal(y[2], [1.0, -2.0]) and L[2, 0] == 5.5          # one edge: its v row, whatever the bias; 2.5 + 3
    # two heads of one column, one bias for both: head 0: e = 0.5 * (3, 0.5) + (0.25, -0.5); head 1: e = 0.5 * (-2, 0) + (0.25, -0.5)
    y, L, _ = dot_attn_bias_ref(ptr, idx, q, k, v, 2, 0.5, np.array([0.25, -0.5, -inf, 3.0], f32))
    b1 = 1.0 / (1.0 + math.exp(-0.25 - 1.75))
    c1 = 1.0 / (1.0 + math.exp(-0.5 + 0.75))
    np.testing.assert_allclose(y[0], [3 * b1 + 0.5 * (1 - b1), -4 * c1 + 8 * (1 - c1)], rtol=1e-14)
    assert np.array_equal(L[0], [1.75, 1.25])         # head 0: max(1.5 + 0.25, 0.25 + 0.5); head 1: max(1 + 0.25, 0 + 0.5)
    # bias_heads = heads: edge 0 masked in head 1, edge 2 in head 0.  head 0: e = (1.5 + 0.5, 0.25 - 1); head 1: e = (0 + 1, 2 + 0.5) on edges 1, 2
    bias = np.array([[0.5, -inf], [-1, 1], [-inf, 0.5], [0, 0]], f32)
    y, L, _ = dot_attn_bias_ref(ptr, idx, q, k, v, 2, 0.5, bias)
    b1 = 1.0 / (1.0 + math.exp(-0.75 - 2.0))
    c1 = 1.0 / (1.0 + math.exp(2.5 - 1.0))            # the weight of edge 1 (v = 8) against edge 2 (source 0, v = -2)
    np.testing.assert_allclose(y[0], [3 * b1 + 0.5 * (1 - b1), 8 * c1 - 2 * (1 - c1)], rtol=1e-14)
    assert np.array_equal(L[0], [2.0, 2.5])           # head 0: max(1.5 + 0.5, 0.25 + 1); head 1: max(0 + 1, 2 + 0.5)
    # a fully masked (row, head) is NaN, a +Inf or NaN bias too; the other head is untouched
    for bad in (-inf, inf, np.nan):
        yb, _, _ = dot_attn_bias_ref(ptr, idx, q, k, v, 2, 0.5, np.array([[0.5, 0], [-1, 0], [-inf, 0], [bad, 0]], f32))
        assert np.isnan(yb[2, 0]) and yb[2, 1] == -2.0 and np.isfinite(yb[0]).all()
    # ---- GATv2: xs, xd, a and slope 0.5 of tests/test_gatv2_host.py; unbiased scores of row 0: 2, 0.5 (and 1 + 0.5 * 2 = 2, masked)
    xs = np.array([[1, 2], [3, -4], [0.5, 0]], f32)
    xd = np.array([[0, 0], [1, 1], [-1, 2]], f32)
    a = np.array([[1, 0.5]], f32)
    y, L, S = gatv2_bias_ref(ptr, idx, xs, xd, a, 1, 0.5, np.array([0.5, -1.0, -inf, 3.0], f32))
    a1 = 1.0 / (1.0 + math.exp(-0.5 - 2.5))            # e = 2.5 and -0.5
    np.testing.assert_allclose(y[0], [3 * a1 + 0.5 * (1 - a1), -4 * a1], rtol=1e-14)
    assert L[0, 0] == 4.5 and np.isfinite(y).all()    # max(4 + 0.5, 0.5 + 1); no column of the masked source is poisoned
    assert np.array_equal(y[2], [1.0, 2.0]) and L[2, 0] == 5.0 and np.all(y[1] == 0)
    # two heads, bias_heads = heads: head 0: e = (3, 0.5, 1), head 1: e = (-1, 0, 1)
    y, L, _ = gatv2_bias_ref(ptr, idx, xs, xd, np.array([[1], [0.5]], f32), 2, 0.5, bias)
    b1 = 1.0 / (1.0 + math.exp(-0.5 - 3.5))            # head 0, edges 0 and 1: 3.5 and -0.5
    c1 = 1.0 / (1.0 + math.exp(1.5 - 1.0))             # head 1, edges 1 and 2: 1 and 1.5; the weight of edge 1 (xs = 0) against edge 2 (xs = 2)
    np.testing.assert_allclose(y[0], [3 * b1 + 0.5 * (1 - b1), 2 * (1 - c1)], rtol=1e-14)
    assert np.array_equal(L[0], [3.5, 1.5])


def test_the_judges_are_block_independent():
    rng = np.random.default_rng(0)
    ptr = np.concatenate([[0], np.cumsum(rng.integers(0, 9, 40))])
    idx = rng.integers(0, 60, ptr[-1])
    q, k, v = (rng.standard_normal((n, 12)).astype(f32) for n in (40, 60, 60))
    a = rng.standard_normal((4, 3)).astype(f32)
    for bias in (rng.standard_normal((ptr[-1], 4)).astype(f32), rng.standard_normal(ptr[-1]).astype(f32)):
        bias[::5] = NINF
        for whole, small in ((dot_attn_bias_ref(ptr, idx, q, k, v, 4, 0.3, bias), dot_attn_bias_ref(ptr, idx, q, k, v, 4, 0.3, bias, block_edges=7)),
                             (gatv2_bias_ref(ptr, idx, k, q, a, 4, 0.2, bias), gatv2_bias_ref(ptr, idx, k, q, a, 4, 0.2, bias, block_edges=7))):
            for x, y in zip(whole, small):
                assert np.array_equal(x, y, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------- the bound
def fp32_scores(call, ptr, idx, ops, H):
    """the score of every (edge, head) as one sequential fp32 chain over the head's columns"""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    F = ops[SCORED[call]].shape[1]
    D = F // H
    e = np.zeros((len(idx), H), f32)
    if call == "dot":
        qs = (ops["q"] * default_scale(D)).astype(f32)
        for c in range(D):
            e = (e + qs[rows, c::D] * ops["k"][idx, c::D]).astype(f32)
        return e
    a = ops["a"].reshape(H, D)
    for c in range(D):
        z = (ops["xd"][rows, c::D] + ops["xs"][idx, c::D]).astype(f32)
        zs = (z * f32(SLOPE)).astype(f32)
        e = (e + a[:, c] * np.where(z > zs, z, zs)).astype(f32)
    return e


def fp32_chain_bias(call, ptr, idx, ops, H, bias):
    """the sequential fp32 chain: the score chain, ONE fp32 add of the bias, then the two-pass softmax in fp32, edge by edge"""
    ptr = np.asarray(ptr, np.int64)
    src = ops["v" if call == "dot" else "xs"]
    n_v, F = len(ptr) - 1, src.shape[1]
    D = F // H
    deg = np.diff(ptr)
    e = (fp32_scores(call, ptr, idx, ops, H) + np.asarray(bias, f32).reshape(len(idx), -1)).astype(f32)
    ne = np.flatnonzero(deg > 0)
    m = np.zeros((n_v, H), f32)
    m[ne] = np.maximum.reduceat(e, ptr[ne], axis=0)
    rows = np.repeat(np.arange(n_v), deg)
    w = np.exp((e - m[rows]).astype(f32)).astype(f32)
    den, acc = np.zeros((n_v, H), f32), np.zeros((n_v, F), f32)
    for t in range(int(deg.max())):
        r = np.flatnonzero(deg > t)
        p = ptr[r] + t
        den[r] = (den[r] + w[p]).astype(f32)
        acc[r] = (acc[r] + (src[idx[p]] * np.repeat(w[p], D, axis=1)).astype(f32)).astype(f32)
    y = np.zeros((n_v, F), f32)
    y[ne] = acc[ne] / np.repeat(den[ne], D, axis=1)
    return y


@pytest.mark.parametrize("call", ["dot", "v2"])
@pytest.mark.parametrize("H,D", SHAPES)
def test_a_sequential_fp32_chain_stays_inside_the_bound(call, H, D):
    ops = case_operands(call, H, D)
    for per_head in (True, False):
        bias = random_bias(H, per_head)
        ref, L, S = bias_ref(call, PTR, IDX, ops, H, bias)
        ratio = worst_ratio(fp32_chain_bias(call, PTR, IDX, ops, H, bias), ref, bias_bound(L, S, H))
        print("fp32 chain, %s %dx%d, bias %s: worst ratio %.4f" % (call, H, D, "[E, H]" if per_head else "[E]", ratio))
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------- the spread
def biased_spread(call, ptr, idx, ops, H, bias, what):
    """assert_spread of tests/test_attn_nonfinite_host.py on the scores with the bias"""
    e = head_scores(call, ptr, idx, ops, H) + np.asarray(bias, np.float64).reshape(len(idx), -1)
    hi, lo = np.where(np.isfinite(e), e, -np.inf), np.where(np.isfinite(e), e, np.inf)
    starts = np.asarray(ptr)[:-1][np.diff(ptr) > 0].astype(np.intp)
    with np.errstate(invalid="ignore"):
        spread = np.maximum.reduceat(hi, starts, axis=0) - np.minimum.reduceat(lo, starts, axis=0)
    worst = float(np.nanmax(np.where(np.isfinite(spread), spread, 0.0))) if spread.size else 0.0
    assert worst < SPREAD, "%s: finite scores of one (row, head) spread by %.1f" % (what, worst)
    return worst


@pytest.mark.parametrize("call", ["dot", "v2"])
@pytest.mark.parametrize("H,D", SHAPES)
def test_the_gpu_files_biased_scores_stay_within_the_spread(call, H, D):
    ops = case_operands(call, H, D)
    for per_head in (True, False):
        worst = biased_spread(call, PTR, IDX, ops, H, random_bias(H, per_head), "%s %dx%d" % (call, H, D))
        print("%s %dx%d, bias %s: widest spread of a (row, head) %.1f" % (call, H, D, "[E, H]" if per_head else "[E]", worst))


# ------------------------------------------------------------------------------------------------------- declared, exported, typed
NEW = {
    "gnnagg_gatv2_run_bias": (r"int gnnagg_gatv2_run_bias\(gnnagg_handle h, const void \*d_xs, const void \*d_xd, int x_dtype, const float \*d_a, "
                              r"void \*d_y, int y_dtype,\s+int feat, int heads, float slope, const float \*d_bias, int bias_heads\);",
                              [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                               ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int]),
    "gnnagg_dot_attn_run_bias": (r"int gnnagg_dot_attn_run_bias\(gnnagg_handle h, const void \*d_q, long long q_pitch, const void \*d_k, "
                                 r"const void \*d_v, long long kv_pitch,\s+int x_dtype, void \*d_y, int y_dtype, int feat, int heads, float scale, "
                                 r"const float \*d_bias, int bias_heads\);",
                                 [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int]),
}


def test_header_declares_and_the_library_exports_the_bias_calls():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, (decl, args) in NEW.items():
        assert re.search(decl, text), name
        assert name in exported
        res, got = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and got == args
        assert getattr(gnc.lib(), name).argtypes == args
    for phrase in ("p * bias_heads + (bias_heads == 1 ? 0 : h)", "a bias of -Inf is a mask", "captured in a HIP graph"):
        assert phrase in text
    # the kernels: the operand pair of the shared arguments, and the arm chosen from the pointer in the one launcher both kernels go through
    csrc = os.path.join(ROOT, "gnn_computing_amd", "csrc")
    shared = open(os.path.join(csrc, "gatv2_shared.cuh")).read()
    assert re.search(r"const float \*bias;.*\n\s*int bias_heads;", shared)
    assert re.search(r"if \(a\.bias\) hipLaunchKernelGGL\(\(K::template get<VEC, GROUP, NF, TX, SEGRED, true, false>\(\)\)", shared)
    assert re.search(r"else hipLaunchKernelGGL\(\(K::template get<VEC, GROUP, NF, TX, SEGRED, false, false>\(\)\)", shared)
    for name, functor, kernel in (("agg_gatv2.hip", "Gatv2Kernel", "k_gatv2"), ("agg_dot.hip", "DotKernel", "k_dot_attn")):
        src = open(os.path.join(csrc, name)).read()
        assert re.search(r"struct %s \{[^}]*return &%s<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS>;" % (functor, kernel), src)
        assert "attn_launch_typed<%s, " % functor in src and "hipLaunchKernelGGL" not in src


# --------------------------------------------------------------------------------------------------------------- Python-side refusals
def _stub_aggregator(monkeypatch, n_v=4, n_e=6):
    """an Aggregator_GAT without a device handle; what passes the checks reaches a library that records the entry point and raises"""
    agg = gnc.Aggregator_GAT.__new__(gnc.Aggregator_GAT)
    agg.num_v, agg.num_e, agg.feat_in, agg.feat_out, agg._h = n_v, n_e, 8, 8, ctypes.c_int64(0)
    reached = []

    class Lib:
        def __getattr__(self, name):
            def entry(*args):
                reached.append((name, args))
                raise _NoDevice()
            return entry
    monkeypatch.setattr(gnc.aggregator, "lib", lambda: Lib())
    monkeypatch.setattr(gnc.aggregator.Aggregator, "_use_current_stream", lambda self: reached.append(("stream", ())))
    monkeypatch.setattr(gnc.aggregator, "_dev_ptr", lambda t, dtype, name: None if t is None else ctypes.c_void_p(t.data_ptr()))
    monkeypatch.setattr(gnc.aggregator, "_dev_ptr_rows", lambda t, dtype, name: (ctypes.c_void_p(t.data_ptr()), int(t.stride(0))))
    return agg, reached


def test_bias_is_checked_before_the_library_is_reached(monkeypatch):
    agg, reached = _stub_aggregator(monkeypatch)
    H, n_e = 2, agg.num_e
    x, a = torch.zeros((4, 8)), torch.zeros(8)
    runs = {"gnnagg_dot_attn_run": [lambda **kw: agg.run_dot(x, x, x, x.clone(), heads=H, **kw), lambda **kw: gnc.dot_attn_run(agg, x, x, x, x.clone(), heads=H, **kw)],
            "gnnagg_gatv2_run": [lambda **kw: agg.run_v2(x, x, a, x.clone(), heads=H, **kw), lambda **kw: gnc.gatv2_run(agg, x, x, a, x.clone(), heads=H, **kw)]}
    for old, forms in runs.items():
        for run in forms:
            for bad in (np.zeros(n_e, np.float32), [0.0] * n_e, 0.0, torch.zeros(n_e, dtype=torch.float64), torch.zeros(n_e, dtype=torch.bfloat16),
                        torch.zeros((n_e, H), dtype=torch.float16), torch.zeros(n_e, dtype=torch.int32)):
                with pytest.raises(TypeError, match="bias"):
                    run(bias=bad)
            for bad in (torch.zeros(n_e + 1), torch.zeros(n_e - 1), torch.zeros((n_e, 3)), torch.zeros((n_e, 2 * H)), torch.zeros((H, n_e)),
                        torch.zeros((n_e, H, 1)), torch.zeros((1, n_e)), torch.zeros(()), torch.zeros((n_e, 0))):
                with pytest.raises(ValueError, match="bias must be"):
                    run(bias=bad)
            for bad in (torch.zeros(2 * n_e)[::2], torch.zeros((n_e, 2 * H))[:, :H], torch.zeros((H, n_e)).t(), torch.zeros((n_e, 2))[:, :1]):
                assert not bad.is_contiguous() or bad.shape == (n_e, 1)
                if not bad.is_contiguous():
                    with pytest.raises(ValueError, match="contiguous"):
                        run(bias=bad)
            assert reached == []          # neither the stream nor the library
            # bias=None: today's entry point; a valid bias: the new one, with bias_heads as the last argument
            with pytest.raises(_NoDevice):
                run()
            with pytest.raises(_NoDevice):
                run(bias=None)
            assert [n for n, _ in reached] == ["stream", old, "stream", old]
            del reached[:]
            for good, bh in ((torch.zeros(n_e), 1), (torch.zeros((n_e, 1)), 1), (torch.zeros((n_e, H)), H),
                             (torch.full((n_e, H), -math.inf), H), (torch.zeros(n_e + 3)[3:], 1)):
                with pytest.raises(_NoDevice):
                    run(bias=good)
                (s, _), (name, args) = reached
                assert s == "stream" and name == old + "_bias" and args[-1] == bh and args[-2].value == good.data_ptr()
                del reached[:]
    # one head: [E, 1] is [E, heads]
    with pytest.raises(_NoDevice):
        agg.run_dot(x, x, x, x.clone(), heads=1, bias=torch.zeros((n_e, 1)))
    assert reached[-1][0] == "gnnagg_dot_attn_run_bias" and reached[-1][1][-1] == 1


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_the_bias_calls_error_out_without_a_gpu():
    L = gnc.lib()
    x, y, b = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.float32)
    rc = L.gnnagg_dot_attn_run_bias(ctypes.c_int64(0), x.ctypes.data, 8, x.ctypes.data, x.ctypes.data, 8, 0, y.ctypes.data, 0, 8, 1,
                                    ctypes.c_float(0.5), b.ctypes.data, 1)
    assert rc == _lib.ERR_ARG and b"handle" in L.gnnagg_last_error()
    rc = L.gnnagg_gatv2_run_bias(ctypes.c_int64(0), x.ctypes.data, x.ctypes.data, 0, x.ctypes.data, y.ctypes.data, 0, 8, 1, ctypes.c_float(0.2),
                                 b.ctypes.data, 1)
    assert rc == _lib.ERR_ARG and b"handle" in L.gnnagg_last_error()
    # no GPU: no handle can be made, and the old entry points say the same
    rc = L.gnnagg_gatv2_run(ctypes.c_int64(0), x.ctypes.data, x.ctypes.data, 0, x.ctypes.data, y.ctypes.data, 0, 8, 1, ctypes.c_float(0.2))
    assert rc == _lib.ERR_ARG and b"handle" in L.gnnagg_last_error()


# ------------------------------------------------------------------------------------------------ the online recurrence, masked by a bias
@pytest.mark.parametrize("pattern", PATTERNS, ids=pattern_id)
def test_the_recurrence_has_the_judges_class_where_a_bias_masks(pattern):
    """the kernels add the bias in fp32 before the batch maximum: a -Inf bias on a finite score IS a -Inf score, and the recurrence of
    tests/test_attn_nonfinite_host.py (emulate_row) then has the class of the float64 judge on every pattern -- with a zero and with a
    random finite bias on the edges that stay.  This pins what tests/test_gpu_attn_bias.py expects of the kernels; it runs no product code."""
    for n in ROW_LENGTHS:
        e, x = one_row(n, n)
        mask = mask_edges(np.array([0, n]), pattern)
        for finite in (np.zeros(n, f32), bf16_exact(2.0 * np.random.default_rng(n).standard_normal(n))):
            bias = finite.copy()
            bias[mask] = NINF
            eb = (e + bias).astype(f32)
            assert np.array_equal(np.isneginf(eb), mask) and np.isfinite(eb[~mask]).all()
            y = check_row(eb, x, "bias mask %s, %d edges" % (pattern_id(pattern), n))
            assert np.isnan(y) == bool(mask.all())
            # the float64 judge with the bias as an operand says the same as the judge on the summed scores
            yb, _, _ = dot_attn_bias_ref(np.array([0, n]), np.arange(n), np.ones((1, 1), f32), e.reshape(-1, 1), x.reshape(-1, 1), 1, 1.0, bias)
            assert classes(yb[0, 0]) == classes(y)
            if np.isfinite(y):
                # (eb is e + bias rounded once to fp32: up to 2^-24 * 32 = 2e-6 on a score, relative on a weight, twice that on y)
                assert abs(yb[0, 0] - y) <= 1e-5 * np.abs(x).max()
    # +Inf and NaN biases: NaN, wherever they stand and behind masked edges
    for n in (1, 5, 9, 130):
        for pos in (0, n // 2, n - 1):
            for bad in (np.inf, np.nan):
                e, x = one_row(n, n)
                bias = np.zeros(n, f32)
                bias[pos] = bad
                assert np.isnan(check_row((e + bias).astype(f32), x, "%r bias at %d of %d" % (bad, pos, n)))
                bias[:pos] = NINF
                assert np.isnan(check_row((e + bias).astype(f32), x, "%r bias at %d of %d behind masks" % (bad, pos, n)))
    assert emulate_row is not None and row_judge is not None and delete_edges is not None
