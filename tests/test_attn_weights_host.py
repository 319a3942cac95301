"""Host: the weights-out form of the two online-softmax attention calls (gnnagg_gatv2_run_weights / Aggregator_GAT.run_v2(weights=, stats=),
gnnagg_dot_attn_run_weights / Aggregator_GAT.run_dot(weights=, stats=)) -- the judges, inputs and expectations of
tests/test_gpu_attn_weights.py, pinned without a GPU.

  * weights_ref: the float64 two-pass formulas of include/gnnagg.h, returning (y, alpha, M, den, L).  y and L are those of the imported
    judges (dot_attn_bias_ref / gatv2_bias_ref, which are dot_attn_ref / gatv2_ref at a zero bias); alpha, M and den come from the same
    float64 scores, and alpha is tied to the judges by running them with v = the indicator of every source;
  * the bound |alpha - ref| <= 1e-5 (1 + L[r, h]) ref -- the project's y bound with S = alpha --, and a sequential fp32 emulation (score
    chain, ONE bias add, the final maximum, expf(e - ms) / den) that stays inside it on every input of the GPU file;
  * the spread condition (finite scores of a (row, head) within 60 of each other: no weight is subnormal) on those inputs;
  * the declarations, the Python-side refusals and the entry point each argument combination reaches."""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import geometry_census as gc
import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_attn_bias_host import (_stub_aggregator, bias_ref, biased_spread, dot_attn_bias_ref, fp32_scores, gatv2_bias_ref,
                                 random_bias)
from test_attn_nonfinite_host import SHAPES, SPREAD, attn_operands, bf16_exact, delete_edges, head_scores, small_graph
from test_dot_attn_host import _NoDevice, dot_attn_bound, dot_attn_ref
from test_gatv2_host import gatv2_ref
from test_gpu_gatv2 import threshold_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
RTOL = 1e-5


# ------------------------------------------------------------------------------------------------------------------- the judge
def softmax_parts(ptr, e):
    """the two-pass float64 softmax of scores e [E, H] over the CSR rows: (alpha [E, H], M [V, H], den [V, H]); a row without edges is
    (-inf, 0); a (row, head) whose scores are all -inf, or hold a +inf or a NaN, is NaN on every edge (IEEE, as the formulas stand)"""
    ptr = np.asarray(ptr, np.int64)
    e = np.asarray(e, np.float64)
    V, H = len(ptr) - 1, e.shape[1]
    deg = np.diff(ptr)
    M, den = np.full((V, H), -np.inf), np.zeros((V, H))
    ne = np.flatnonzero(deg > 0)
    if len(ne) == 0:
        return np.zeros((0, H)), M, den
    starts = ptr[ne].astype(np.intp)
    rows = np.repeat(np.arange(V), deg)
    with np.errstate(all="ignore"):
        M[ne] = np.fmax.reduceat(e, starts, axis=0)            # (fmax: a NaN score does not hide the others' maximum; den is NaN anyway)
        M[np.isnan(M)] = -np.inf
        w = np.exp(e - np.where(np.isneginf(M), 0.0, M)[rows])  # (all -inf: exp(-inf - 0) = 0 on every edge, 0 / 0 below)
        den[ne] = np.add.reduceat(w, starts, axis=0)
        alpha = w / den[rows]
    return alpha, M, den


def weights_ref(call, ptr, idx, ops, H, bias=None):
    """(y, alpha, M, den, L) of one call on the operands of attn_operands (default scale, slope 0.2); bias None, [E] or [E, H]"""
    n_e = len(idx)
    b = np.zeros(n_e, f32) if bias is None else np.asarray(bias, f32)
    y, L, _ = bias_ref(call, ptr, idx, ops, H, b)
    e = head_scores(call, ptr, idx, ops, H) + b.astype(np.float64).reshape(n_e, -1)
    alpha, M, den = softmax_parts(ptr, e)
    return y, alpha, M, den, L


def alpha_bound(alpha_ref, L, ptr):
    """|alpha - ref| <= 1e-5 (1 + L[r, h]) ref: the y bound 1e-5 (1 + L) S with v the indicator of one edge's source (S = alpha)"""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return RTOL * (1.0 + L[rows]) * alpha_ref


def stat_bounds(M_ref, den_ref, L):
    """(|M - ref| allowed, |den - ref| allowed): 1e-5 (1 + L) absolute on the maximum, the same factor relative on the denominator"""
    return RTOL * (1.0 + L), RTOL * (1.0 + L) * den_ref


def ratio(got, ref, bound):
    """max |got - ref| / bound where ref is finite; 0 / 0 counts as 0, x / 0 as inf"""
    ok = np.isfinite(ref)
    err = np.abs(np.asarray(got, np.float64)[ok] - ref[ok])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound[ok])
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0


def test_the_bound_is_the_projects_own_with_alpha_for_s():
    ptr = np.array([0, 2, 2, 3])
    L, alpha = np.array([[1.0, 3.0], [0.0, 0.0], [2.0, 0.5]]), np.array([[0.25, 0.5], [0.75, 0.5], [1.0, 1.0]])
    want = dot_attn_bound(L[[0, 0, 2]], alpha, 2)       # heads of one column: S [E, H] is alpha itself
    assert np.array_equal(alpha_bound(alpha, L, ptr), want)
    assert np.allclose(alpha_bound(alpha, L, ptr), 1e-5 * np.array([[2 * 0.25, 4 * 0.5], [2 * 0.75, 4 * 0.5], [3.0, 1.5]]))


def test_alpha_is_the_judges_y_with_an_indicator_for_v():
    """one head of n_src columns and v = the identity: y[r, s] of the imported judges IS the sum of the row's weights on source s"""
    ptr, idx, n_src = small_graph()
    V, E = len(ptr) - 1, len(idx)
    rng = np.random.default_rng(5)
    q, k = bf16_exact(rng.standard_normal((V, n_src)) / 4), bf16_exact(rng.standard_normal((n_src, n_src)) / 4)
    bias = bf16_exact(rng.standard_normal(E))
    bias[3::7] = -np.inf           # (no row is masked whole: the rows of one and two edges come first)
    eye = np.eye(n_src, dtype=f32)
    rows = np.repeat(np.arange(V), np.diff(ptr))
    scale = f32(0.25)
    for b in (np.zeros(E, f32), bias):
        y, L, S = dot_attn_bias_ref(ptr, idx, q, k, eye, 1, scale, b)
        e = float(scale) * (q.astype(np.float64)[rows] * k.astype(np.float64)[idx]).sum(axis=1, keepdims=True) + b.astype(np.float64)[:, None]
        alpha, M, den = softmax_parts(ptr, e)
        got = np.zeros((V, n_src))
        np.add.at(got, (rows, idx), alpha[:, 0])
        np.testing.assert_allclose(got, y, rtol=1e-13, atol=0)
        assert np.array_equal(alpha[:, 0] == 0, np.isneginf(b)) and np.allclose(np.add.reduceat(alpha[:, 0], ptr[:-1][np.diff(ptr) > 0]), 1)
    # a zero bias is the unbiased judge; GATv2 likewise
    assert np.array_equal(dot_attn_bias_ref(ptr, idx, q, k, eye, 1, scale, np.zeros(E, f32))[0], dot_attn_ref(ptr, idx, q, k, eye, 1, scale)[0])
    a = bf16_exact(rng.standard_normal((1, n_src)) / 4)
    assert np.array_equal(gatv2_bias_ref(ptr, idx, k, q, a, 1, 0.2, np.zeros(E, f32))[0], gatv2_ref(ptr, idx, k, q, a, 1, 0.2)[0])


def test_the_judge_on_a_hand_computed_example_and_its_non_finite_classes():
    # rows: 0 -> {1, 2, 0}, 1 -> {}, 2 -> {0}; scores of row 0: 0.5, 0.25, 2.5 (tests/test_attn_bias_host.py)
    ptr = np.array([0, 3, 3, 4])
    e = np.array([[0.5], [0.25], [2.5], [7.0]])
    alpha, M, den = softmax_parts(ptr, e)
    d = math.exp(-2.0) + math.exp(-2.25) + 1.0
    np.testing.assert_allclose(alpha[:, 0], [math.exp(-2.0) / d, math.exp(-2.25) / d, 1 / d, 1.0], rtol=1e-15)
    assert M[0, 0] == 2.5 and math.isclose(den[0, 0], d, rel_tol=1e-15) and np.isneginf(M[1, 0]) and den[1, 0] == 0 and not np.signbit(den[1, 0])
    assert M[2, 0] == 7.0 and den[2, 0] == 1.0 and alpha[3, 0] == 1.0
    # a masked edge is +0 and the others are the row without it; all masked: NaN with (-inf, 0); +inf and NaN: NaN on every edge
    e2 = e.copy()
    e2[2] = -np.inf
    a2, M2, d2 = softmax_parts(ptr, e2)
    ptr_d, _ = delete_edges(ptr, np.arange(4), np.array([False, False, True, False]))[:2]
    a3, M3, d3 = softmax_parts(ptr_d, e[[0, 1, 3]])
    assert a2[2, 0] == 0 and not np.signbit(a2[2, 0]) and np.array_equal(a2[[0, 1, 3]], a3) and np.array_equal(M2, M3) and np.array_equal(d2, d3)
    a4, M4, d4 = softmax_parts(ptr, np.array([[-np.inf]] * 3 + [[1.0]]))
    assert np.isnan(a4[:3]).all() and a4[3, 0] == 1 and np.isneginf(M4[0, 0]) and d4[0, 0] == 0
    for bad in (np.inf, np.nan):
        a5, _, d5 = softmax_parts(ptr, np.array([[0.5], [bad], [-np.inf], [1.0]]))
        assert np.isnan(a5[:3]).all() and np.isnan(d5[0, 0]) and a5[3, 0] == 1 and d5[2, 0] == 1


# ------------------------------------------------------------------------------------------------------------------- the inputs
PTR, IDX, N_SRC = threshold_graph(n_src_extra=300)
V, E = len(PTR) - 1, len(IDX)
DEG = np.diff(PTR)
ROWS = np.repeat(np.arange(V), DEG)
CENSUS = sorted(gc.GATV2)
BIAS_FORMS = ("none", "edge", "head")
CALLS = ("dot", "v2")


def test_the_graph_has_the_row_lengths_the_kernels_switch_at():
    assert 30 <= V <= 48
    for n in (0, 1, 3, 4, 5, 127, 128, 129, 512, 513, 1025):
        assert (DEG == n).any(), n
    assert (DEG > 3 * 512).any()        # four segments: the merge folds more than three


def census_operands(call, H, D):
    """the operands of the GPU file's geometry cases (bf16-exact: one set serves the fp32 run, the bf16 run and the judge; read-only)"""
    return attn_operands(call, V, N_SRC, H, D, H // 2, seed=H * D + 1)


def case_bias(form, H):
    """the bias of one form on the threshold graph: None, [E] or [E, H] (bf16-exact 2 * randn, read-only)"""
    return None if form == "none" else random_bias(H, form == "head", E)


@functools.lru_cache(maxsize=4)
def census_ref(call, H, D):
    """weights_ref of one geometry case, computed once and shared (read-only)"""
    out = weights_ref(call, PTR, IDX, census_operands(call, H, D), H)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=8)
def bias_case_ref(call, H, D, form):
    out = weights_ref(call, PTR, IDX, census_operands(call, H, D), H, case_bias(form, H))
    for x in out:
        x.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------- the bound
def fp32_weights(call, ptr, idx, ops, H, bias):
    """the arithmetic of the weights call as one sequential fp32 emulation: the score chain, ONE fp32 add of the bias, the row's final
    maximum M, the denominator summed edge by edge, alpha = expf(e - ms) / den with ms = M (0 where M is -inf).  Returns (alpha, M, den)."""
    ptr = np.asarray(ptr, np.int64)
    n_v = len(ptr) - 1
    deg = np.diff(ptr)
    e = fp32_scores(call, ptr, idx, ops, H)
    if bias is not None:
        e = (e + np.asarray(bias, f32).reshape(len(idx), -1)).astype(f32)
    ne = np.flatnonzero(deg > 0)
    M = np.full((n_v, H), -np.inf, f32)
    M[ne] = np.maximum.reduceat(e, ptr[ne], axis=0)
    rows = np.repeat(np.arange(n_v), deg)
    with np.errstate(all="ignore"):
        ms = np.where(np.isneginf(M), f32(0), M)
        w = np.exp((e - ms[rows]).astype(f32)).astype(f32)
        den = np.zeros((n_v, H), f32)
        for t in range(int(deg.max()) if len(deg) else 0):
            r = np.flatnonzero(deg > t)
            den[r] = (den[r] + w[ptr[r] + t]).astype(f32)
        alpha = (w / den[rows]).astype(f32)
    return alpha, M, den


def check_against(got, ref, ptr, what):
    """(alpha, M, den) against weights_ref's (y, alpha, M, den, L): the three ratios, asserted <= 1"""
    alpha, M, den = got
    _, a_ref, M_ref, d_ref, L = ref
    mb, db = stat_bounds(M_ref, d_ref, L)
    has = np.diff(ptr) > 0
    r = (ratio(alpha, a_ref, alpha_bound(a_ref, L, ptr)), ratio(M[has], M_ref[has], mb[has]), ratio(den[has], d_ref[has], db[has]))
    print("%s: fractions of the bound: alpha %.4f, M %.4f, den %.4f" % ((what,) + r))
    assert max(r) <= 1.0, what
    return r


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("H,D", CENSUS)
def test_a_sequential_fp32_emulation_stays_inside_the_bound_on_the_geometry_cases(call, H, D):
    ops = census_operands(call, H, D)
    worst = biased_spread(call, PTR, IDX, ops, H, np.zeros(E, f32), "%s %dx%d" % (call, H, D))
    assert worst < SPREAD
    check_against(fp32_weights(call, PTR, IDX, ops, H, None), census_ref(call, H, D), PTR, "fp32 emulation, %s %dx%d" % (call, H, D))


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("H,D", SHAPES)
def test_a_sequential_fp32_emulation_stays_inside_the_bound_on_the_bias_cases(call, H, D):
    ops = census_operands(call, H, D)
    for form in BIAS_FORMS[1:]:
        bias = case_bias(form, H)
        assert biased_spread(call, PTR, IDX, ops, H, bias, "%s %dx%d %s" % (call, H, D, form)) < SPREAD
        check_against(fp32_weights(call, PTR, IDX, ops, H, bias), weights_ref(call, PTR, IDX, ops, H, bias), PTR,
                      "fp32 emulation, %s %dx%d, bias per %s" % (call, H, D, form))


def test_the_emulation_has_the_judges_classes_under_masks_and_non_finite_scores():
    ptr, idx, n_src = small_graph()
    n_v, n_e = len(ptr) - 1, len(idx)
    H, D = 3, 4
    for call in CALLS:
        ops = attn_operands(call, n_v, n_src, H, D, 1, seed=9)
        for bad in (-np.inf, np.inf, np.nan):
            bias = np.zeros((n_e, H), f32)
            bias[::3, 1] = bad
            bias[ptr[4]:ptr[5], 2] = -np.inf            # one (row, head) all masked
            got = fp32_weights(call, ptr, idx, ops, H, bias)
            ref = weights_ref(call, ptr, idx, ops, H, bias)
            assert np.array_equal(np.isnan(got[0]), np.isnan(ref[1])) and np.array_equal(got[0] == 0, ref[1] == 0)
            assert not np.signbit(got[0][got[0] == 0]).any()
            assert np.isnan(got[0][ptr[4]:ptr[5], 2]).all() and np.isneginf(got[1][4, 2]) and got[2][4, 2] == 0
            fin = np.isfinite(ref[1])
            assert ratio(np.where(fin, got[0], 0), np.where(fin, ref[1], 0), alpha_bound(np.where(fin, ref[1], 0), ref[4], ptr)) <= 1.0


# ------------------------------------------------------------------------------------------------------- declared, exported, typed
I64, P, I, F = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_float
NEW = {
    "gnnagg_gatv2_run_weights": (r"int gnnagg_gatv2_run_weights\(gnnagg_handle h, const void \*d_xs, const void \*d_xd, int x_dtype, const float \*d_a, "
                                 r"void \*d_y, int y_dtype,\s+int feat, int heads, float slope, const float \*d_bias, int bias_heads, "
                                 r"float \*d_alpha, float \*d_stat\);",
                                 [I64, P, P, I, P, P, I, I, I, F, P, I, P, P]),
    "gnnagg_dot_attn_run_weights": (r"int gnnagg_dot_attn_run_weights\(gnnagg_handle h, const void \*d_q, long long q_pitch, const void \*d_k, "
                                    r"const void \*d_v, long long kv_pitch,\s+int x_dtype, void \*d_y, int y_dtype, int feat, int heads, "
                                    r"float scale, const float \*d_bias, int bias_heads,\s+float \*d_alpha, float \*d_stat\);",
                                    [I64, P, I64, P, P, I64, I, P, I, I, I, F, P, I, P, P]),
}


def test_header_declares_and_the_library_exports_the_weights_calls():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, (decl, args) in NEW.items():
        assert re.search(decl, text), name
        assert name in exported
        res, got = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and got == args
        assert getattr(gnc.lib(), name).argtypes == args
        # the arguments of the _bias call, then the two outputs
        assert got[:-2] == _lib.SIGNATURES[name.replace("_weights", "_bias")][1]
    for phrase in ("alpha[p, h] = expf(e_p - ms) / den", "stat[r, h, 0] = M, stat[r, h, 1] = den", "(-Inf, +0)", "no handle state is added"):
        assert phrase in text, phrase
    # the kernels: the arm is chosen from the pointer in the one launcher both kernels go through, ahead of the two existing arms, and adds no
    # case label
    csrc = os.path.join(ROOT, "gnn_computing_amd", "csrc")
    shared = open(os.path.join(csrc, "gatv2_shared.cuh")).read()
    assert re.search(r"float \*alpha;.*\n\s*float \*stat;", shared)
    assert re.search(r"if \(a\.alpha\) hipLaunchKernelGGL\(\(K::template get<VEC, GROUP, NF, TX, SEGRED, true, true>\(\)\)", shared)
    arms = re.findall(r"(if \(a\.alpha\)|else if \(a\.bias\)|else) hipLaunchKernelGGL\(\(K::template get<", shared)
    assert arms == ["if (a.alpha)", "else if (a.bias)", "else"]                       # none, BIAS, BIAS + WEIGHTS: no full product
    for name, functor, kernel in (("agg_gatv2.hip", "Gatv2Kernel", "k_gatv2"), ("agg_dot.hip", "DotKernel", "k_dot_attn")):
        src = open(os.path.join(csrc, name)).read()
        assert re.search(r"struct %s \{[^}]*return &%s<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS>;" % (functor, kernel), src)
        assert "attn_launch_typed<%s, " % functor in src and "hipLaunchKernelGGL" not in src
    assert "k_attn_finish" in open(os.path.join(csrc, "aux_kernels.hip")).read()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_the_weights_calls_error_out_without_a_gpu():
    L = gnc.lib()
    x, y, w, s = (np.zeros(8, np.float32) for _ in range(4))
    rc = L.gnnagg_dot_attn_run_weights(ctypes.c_int64(0), x.ctypes.data, 8, x.ctypes.data, x.ctypes.data, 8, 0, y.ctypes.data, 0, 8, 1,
                                       ctypes.c_float(0.5), None, 1, w.ctypes.data, s.ctypes.data)
    assert rc == _lib.ERR_ARG and b"handle" in L.gnnagg_last_error()
    rc = L.gnnagg_gatv2_run_weights(ctypes.c_int64(0), x.ctypes.data, x.ctypes.data, 0, x.ctypes.data, y.ctypes.data, 0, 8, 1,
                                    ctypes.c_float(0.2), None, 1, w.ctypes.data, s.ctypes.data)
    assert rc == _lib.ERR_ARG and b"handle" in L.gnnagg_last_error()


# --------------------------------------------------------------------------------------------------------------- Python-side refusals
def test_weights_and_stats_are_checked_before_the_library_is_reached(monkeypatch):
    agg, reached = _stub_aggregator(monkeypatch)
    H, n_e, n_v = 2, agg.num_e, agg.num_v
    x, a = torch.zeros((4, 8)), torch.zeros(8)
    runs = {"gnnagg_dot_attn_run": [lambda **kw: agg.run_dot(x, x, x, x.clone(), heads=H, **kw), lambda **kw: gnc.dot_attn_run(agg, x, x, x, x.clone(), heads=H, **kw)],
            "gnnagg_gatv2_run": [lambda **kw: agg.run_v2(x, x, a, x.clone(), heads=H, **kw), lambda **kw: gnc.gatv2_run(agg, x, x, a, x.clone(), heads=H, **kw)]}
    w_ok, s_ok = torch.zeros((n_e, H)), torch.zeros((n_v, H, 2))
    for old, forms in runs.items():
        for run in forms:
            for bad in (np.zeros((n_e, H), np.float32), [0.0] * n_e, 0.0, torch.zeros((n_e, H), dtype=torch.float64),
                        torch.zeros((n_e, H), dtype=torch.bfloat16), torch.zeros((n_e, H), dtype=torch.int32)):
                with pytest.raises(TypeError, match="weights"):
                    run(weights=bad)
                with pytest.raises(TypeError, match="stats"):
                    run(weights=w_ok, stats=bad)
            for bad in (torch.zeros(n_e), torch.zeros((n_e, 1)), torch.zeros(n_e * H), torch.zeros((n_e + 1, H)), torch.zeros((n_e, H + 1)),
                        torch.zeros((H, n_e)), torch.zeros((n_e, H, 1)), torch.zeros(())):
                with pytest.raises(ValueError, match="weights must be"):
                    run(weights=bad)
            for bad in (torch.zeros((n_v, H)), torch.zeros((n_v, H, 1)), torch.zeros((n_v + 1, H, 2)), torch.zeros((n_v, H + 1, 2)),
                        torch.zeros(n_v * H * 2), torch.zeros((2, H, n_v))):
                with pytest.raises(ValueError, match="stats must be"):
                    run(weights=w_ok, stats=bad)
            for bad_w, bad_s in ((torch.zeros((n_e, 2 * H))[:, :H], None), (torch.zeros((H, n_e)).t(), None), (w_ok, torch.zeros((n_v, H, 4))[:, :, :2]),
                                 (w_ok, torch.zeros((n_v, 2, H)).transpose(1, 2))):
                with pytest.raises(ValueError, match="contiguous"):
                    run(weights=bad_w, stats=bad_s)
            with pytest.raises(ValueError, match="stats without weights"):
                run(stats=s_ok)
            with pytest.raises(ValueError, match="stats without weights"):
                run(weights=None, stats=s_ok, bias=torch.zeros(n_e))
            # a bad bias is still refused with weights given
            with pytest.raises(ValueError, match="bias must be"):
                run(weights=w_ok, stats=s_ok, bias=torch.zeros(n_e + 1))
            assert reached == []          # neither the stream nor the library
            # None / None: today's entry points, with and without a bias
            with pytest.raises(_NoDevice):
                run()
            with pytest.raises(_NoDevice):
                run(weights=None, stats=None)
            with pytest.raises(_NoDevice):
                run(bias=torch.zeros(n_e), weights=None, stats=None)
            assert [n for n, _ in reached] == ["stream", old, "stream", old, "stream", old + "_bias"]
            del reached[:]
            # weights: the new entry point -- the bias pointer (null without one) and bias_heads, then the two outputs
            for bias, bh in ((None, 1), (torch.zeros(n_e), 1), (torch.zeros((n_e, H)), H)):
                for stats in (s_ok, None):
                    with pytest.raises(_NoDevice):
                        run(weights=w_ok, stats=stats, bias=bias)
                    (s, _), (name, args) = reached
                    assert s == "stream" and name == old + "_weights"
                    assert args[-2].value == w_ok.data_ptr() and args[-3] == bh
                    assert (args[-4] is None) if bias is None else (args[-4].value == bias.data_ptr())
                    if stats is not None:
                        assert args[-1].value == s_ok.data_ptr()
                    else:
                        assert args[-1].value not in (None, 0, s_ok.data_ptr())        # allocated by the wrapper
                    del reached[:]
    # one head: [E] serves as [E, 1]
    for w in (torch.zeros(n_e), torch.zeros((n_e, 1))):
        with pytest.raises(_NoDevice):
            agg.run_dot(x, x, x, x.clone(), heads=1, weights=w)
        assert reached[-1][0] == "gnnagg_dot_attn_run_weights" and reached[-1][1][-2].value == w.data_ptr()
