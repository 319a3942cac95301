"""Host: the per-edge feature vectors of the two online-softmax attention calls (gnnagg_gatv2_run_edge / Aggregator_GAT.run_v2(edge=),
gnnagg_dot_attn_run_edge / Aggregator_GAT.run_dot(edge=)) -- the judges, inputs and expectations of tests/test_gpu_attn_edge.py, pinned
without a GPU.

  * dot_attn_edge_ref / gatv2_edge_ref: the float64 two-pass formulas of include/gnnagg.h with SEPARATE scored and summed rows per edge:
    the dot-product scores k[j] + ef[p] and sums v[j] + ef[p]; GATv2 scores xs[j] + ef[p] and sums xs[j].  They return (y, L, S) with L
    taken over the scores with ef (and the bias) and S = sum alpha |summed row|.  With ef = 0 they are dot_attn_ref / gatv2_ref exactly;
    on the expanded graph (ptr, arange(E)) they are dot_attn_ref of the materialised rows; and they agree with an example worked by hand;
  * the bound 1e-5 (1 + L) S, and a sequential fp32 emulation (ONE fp32 add per element, then the fp32 chains of
    tests/test_attn_bias_host.py) that stays inside it on every shape of SHAPES -- so the bound is neither vacuous nor unreachable;
  * the declarations, the exports, the ctypes table; the Python-side refusals on a stubbed aggregator; the calls without a GPU; the
    example's --edge-dim flag."""
import ctypes
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_attn_bias_host import (E, IDX, N_SRC, PTR, V, _bias_ref, _stub_aggregator, bias_bound, case_operands, fp32_chain_bias, fp32_scores,
                                 random_bias)
from test_attn_nonfinite_host import SCORED, SHAPES, SLOPE, attn_operands, bf16_exact, default_scale, full_ref, small_graph
from test_dot_attn_host import _NoDevice, dot_attn_bound, dot_attn_ref
from test_gatv2_host import gatv2_bound, gatv2_ref, worst_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ARANGE = np.arange(E, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------- the judges
def _edge_ref(ptr, t, mult, s, heads, bias=None):
    """the two-pass float64 softmax and sum over the rows of ptr, from per-edge arrays: scores mult * sum_c t[p] (+ bias[p, h]) and summed
    rows s[p] ([E, F] float64 each).  Returns (y [V, F], L [V, heads], S [V, F]): the judge of tests/test_attn_bias_host.py on the graph
    (ptr, arange(E)), whose every edge has its own source row -- the scored one (inside t) and the summed one (s) need not be the same."""
    n_e = len(t)
    b = np.zeros(n_e, f32) if bias is None else bias
    return _bias_ref(ptr, np.arange(n_e), lambda rows, cols: (t[cols], mult), s, heads, b, max(n_e, 1))


def _rows_of(ptr):
    return np.repeat(np.arange(len(ptr) - 1), np.diff(np.asarray(ptr, np.int64)))


def dot_attn_edge_ref(ptr, idx, q, k, v, ef, heads, scale, bias=None):
    """float64: k'_p = k[j] + ef[p], v'_p = v[j] + ef[p]; e_p = scale * sum_c q[r, c] k'_p[c] (+ bias); y[r] = sum_p alpha_p v'_p.
    L[r, h] = max_p (|scale| sum_c |q k'| + |bias|), S[r] = sum_p alpha_p |v'_p|."""
    idx = np.asarray(idx, np.int64)
    e64 = np.asarray(ef, np.float64)
    kp, vp = np.asarray(k, np.float64)[idx] + e64, np.asarray(v, np.float64)[idx] + e64
    return _edge_ref(ptr, np.asarray(q, np.float64)[_rows_of(ptr)] * kp, float(f32(scale)), vp, heads, bias)


def gatv2_edge_ref(ptr, idx, xs, xd, a, ef, heads, slope, bias=None):
    """float64: z = xd[r] + (xs[j] + ef[p]); e_p = sum_c a[h, c] leaky(z) (+ bias); y[r] = sum_p alpha_p xs[j] -- the summed row has no ef.
    L[r, h] = max_p (sum_c |a leaky(z)| + |bias|), S[r] = sum_p alpha_p |xs[j]|."""
    idx = np.asarray(idx, np.int64)
    xs64 = np.asarray(xs, np.float64)
    z = np.asarray(xd, np.float64)[_rows_of(ptr)] + (xs64[idx] + np.asarray(ef, np.float64))
    zs = z * float(f32(slope))
    return _edge_ref(ptr, np.asarray(a, np.float64).reshape(1, -1) * np.where(z > zs, z, zs), 1.0, xs64[idx], heads, bias)


def edge_ref(call, ptr, idx, ops, H, ef, bias=None):
    """the judge of one call on the operands of attn_operands (default scale, slope 0.2): (y, L, S)"""
    D = ops[SCORED[call]].shape[1] // H
    with np.errstate(all="ignore"):
        if call == "dot":
            return dot_attn_edge_ref(ptr, idx, ops["q"], ops["k"], ops["v"], ef, H, default_scale(D), bias)
        return gatv2_edge_ref(ptr, idx, ops["xs"], ops["xd"], ops["a"], ef, H, SLOPE, bias)


def edge_bound(L, S, heads):
    """the project's bound: 1e-5 * (1 + L[r, h]) * S[r, hD + c]"""
    return bias_bound(L, S, heads)


def test_the_bound_is_the_projects_own():
    L, S = np.array([[1.0, 3.0]]), np.array([[1.0, 2.0, 3.0, 4.0]])
    assert np.array_equal(edge_bound(L, S, 2), gatv2_bound(L, S, 2)) and np.array_equal(edge_bound(L, S, 2), dot_attn_bound(L, S, 2))


# ------------------------------------------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def _edge_rows(n_e, F, seed):
    ef = bf16_exact(np.random.default_rng(seed).standard_normal((n_e, F), dtype=np.float32))
    ef.setflags(write=False)
    return ef


def edge_rows(H, D, n_e=E):
    """bf16-exact randn [n_e, F]: a distinct row per edge; shared, read-only"""
    return _edge_rows(n_e, H * D, 9000 + H * D)


def expanded(call, idx, ops, ef):
    """the operands of the expanded graph (ptr, arange(E)): every edge's own source row, materialised by ONE fp32 add per element"""
    out = dict(ops)
    if call == "dot":
        out["k"], out["v"] = (ops["k"][idx] + ef).astype(f32), (ops["v"][idx] + ef).astype(f32)
    else:
        out["xs"] = (ops["xs"][idx] + ef).astype(f32)
    return out


def test_zero_edge_rows_are_the_judges_without_them_exactly():
    ptr, idx, n_src = small_graph()
    n_v = len(ptr) - 1
    for H, D in ((3, 4), (1, 8)):
        zero = np.zeros((len(idx), H * D), f32)
        for call in ("dot", "v2"):
            ops = attn_operands(call, n_v, n_src, H, D, 0, seed=40)
            for a, b in zip(edge_ref(call, ptr, idx, ops, H, zero), full_ref(call, ptr, idx, ops, H)):
                assert np.array_equal(a, b)


def test_the_judges_are_the_plain_judge_on_the_expanded_graph():
    ptr, idx, n_src = small_graph()
    n_v, n_e = len(ptr) - 1, len(idx)
    ar = np.arange(n_e)
    for H, D in ((3, 4), (1, 8)):
        ef = edge_rows(H, D, n_e)
        ops = attn_operands("dot", n_v, n_src, H, D, 0, seed=41)
        kp, vp = ops["k"].astype(np.float64)[idx] + ef, ops["v"].astype(np.float64)[idx] + ef
        for a, b in zip(dot_attn_edge_ref(ptr, idx, ops["q"], ops["k"], ops["v"], ef, H, default_scale(D)),
                        dot_attn_ref(ptr, ar, ops["q"], kp, vp, H, default_scale(D))):
            assert np.array_equal(a, b)
        # GATv2: the scores (and L) of the expanded judge; y and S differ by design (the summed row has no ef)
        ops = attn_operands("v2", n_v, n_src, H, D, 0, seed=41)
        xp = ops["xs"].astype(np.float64)[idx] + ef
        got, want = gatv2_edge_ref(ptr, idx, ops["xs"], ops["xd"], ops["a"], ef, H, SLOPE), gatv2_ref(ptr, ar, xp, ops["xd"], ops["a"], H, SLOPE)
        assert np.array_equal(got[1], want[1]) and not np.array_equal(got[0], want[0])
        # ... and summing the expanded rows instead gives the expanded judge's y
        z = ops["xd"].astype(np.float64)[_rows_of(ptr)] + xp
        zs = z * float(f32(SLOPE))
        y, _, S = _edge_ref(ptr, ops["a"].astype(np.float64).reshape(1, -1) * np.where(z > zs, z, zs), 1.0, xp, H)
        assert np.array_equal(y, want[0]) and np.array_equal(S, want[2])


def test_the_judges_agree_with_a_hand_computed_example():
    # rows: 0 -> {1, 2}, 1 -> {}, 2 -> {0}; one head of two columns; the operands of tests/test_dot_attn_host.py / test_gatv2_host.py
    ptr, idx = np.array([0, 2, 2, 3]), np.array([1, 2, 0])
    ef = np.array([[0, 1], [0.5, 0], [1, 1]], f32)
    q = np.array([[1, 2], [5, 5], [-1, 2]], f32)
    k = np.array([[1, 2], [3, -1], [0.5, 0]], f32)
    v = np.array([[1, -2], [3, -4], [0.5, 8]], f32)
    y, L, S = dot_attn_edge_ref(ptr, idx, q, k, v, ef, 1, 0.5)
    # row 0: k' = (3, 0) and (1, 0) -> e = 1.5 and 0.5;  v' = (3, -3) and (1, 8)
    a1 = 1.0 / (1.0 + math.exp(-1.0))
    a2 = 1.0 - a1
    np.testing.assert_allclose(y[0], [3 * a1 + a2, -3 * a1 + 8 * a2], rtol=1e-14)
    np.testing.assert_allclose(S[0], [3 * a1 + a2, 3 * a1 + 8 * a2], rtol=1e-14)
    assert L[0, 0] == 1.5
    assert np.all(y[1] == 0) and not np.signbit(y[1]).any() and L[1, 0] == 0 and np.all(S[1] == 0)
    # row 2: k' = (2, 3), q = (-1, 2): q k' = (-2, 6) -> L = 0.5 * 8; one edge -> v' = (2, -1) exactly
    assert np.array_equal(y[2], [2.0, -1.0]) and L[2, 0] == 4.0 and np.array_equal(S[2], [2.0, 1.0])
    # with a bias: e = 1.5 + 0.25 and 0.5 - 0.75; the third edge's bias widens its L
    y, L, _ = dot_attn_edge_ref(ptr, idx, q, k, v, ef, 1, 0.5, np.array([0.25, -0.75, 3.0], f32))
    b1 = 1.0 / (1.0 + math.exp(-2.0))
    np.testing.assert_allclose(y[0], [3 * b1 + (1 - b1), -3 * b1 + 8 * (1 - b1)], rtol=1e-14)
    assert L[0, 0] == 1.75 and L[2, 0] == 7.0
    # GATv2, slope 0.5: row 0: xs' = (3, -3) and (1, 0), xd = 0 -> l = (3, -1.5) and (1, 0) -> e = 3 - 0.75 and 1; the sum is over xs
    xs = np.array([[1, 2], [3, -4], [0.5, 0]], f32)
    xd = np.array([[0, 0], [1, 1], [-1, 2]], f32)
    a = np.array([[1, 0.5]], f32)
    y, L, S = gatv2_edge_ref(ptr, idx, xs, xd, a, ef, 1, 0.5)
    c1 = 1.0 / (1.0 + math.exp(-1.25))
    np.testing.assert_allclose(y[0], [3 * c1 + 0.5 * (1 - c1), -4 * c1], rtol=1e-14)
    np.testing.assert_allclose(S[0], [3 * c1 + 0.5 * (1 - c1), 4 * c1], rtol=1e-14)
    assert L[0, 0] == 3.75
    # row 2: xs' = (2, 3), xd = (-1, 2) -> z = (1, 5) -> e = 1 + 2.5; y is xs[0] itself
    assert np.array_equal(y[2], [1.0, 2.0]) and L[2, 0] == 3.5 and np.all(y[1] == 0)
    # non-finite ef: -Inf in the scored column masks the edge (dot: and poisons that column of v'); NaN makes the row NaN
    bad = ef.copy()
    bad[0, 0] = -np.inf
    with np.errstate(all="ignore"):
        y, _, _ = dot_attn_edge_ref(ptr, idx, q, k, v, bad, 1, 0.5)
        assert np.isnan(y[0, 0]) and y[0, 1] == 8.0 and np.array_equal(y[2], [2.0, -1.0])      # 0 * -Inf in column 0; the other edge alone
        y, _, _ = gatv2_edge_ref(ptr, idx, xs, xd, a, bad, 1, 0.5)
        assert np.array_equal(y[0], [0.5, 0.0])                                                # xs[2] alone: the summed row is finite
        bad[0, 0] = np.nan
        assert np.isnan(dot_attn_edge_ref(ptr, idx, q, k, v, bad, 1, 0.5)[0][0]).all()


# ------------------------------------------------------------------------------------------------------------------- the bound
def fp32_chain_edge(call, ptr, idx, ops, H, ef):
    """the sequential fp32 emulation: ONE fp32 add per element (k', v' / xs'), then the fp32 chains of tests/test_attn_bias_host.py --
    the score chain on the expanded graph, then its two-pass softmax and sum (through its bias argument, over scores of zero: the dot-product
    sums v', GATv2 the source rows without ef)"""
    ar = np.arange(len(idx), dtype=np.int32)
    exp_ops = expanded(call, idx, ops, ef)
    zero = np.zeros(len(idx), f32)
    if call == "dot":
        return fp32_chain_bias("dot", ptr, ar, exp_ops, H, zero)
    e = fp32_scores("v2", ptr, ar, exp_ops, H)
    mute = dict(ops, a=np.zeros_like(ops["a"]))                 # scores of +0 + e = e exactly
    return fp32_chain_bias("v2", ptr, idx, mute, H, e)


@pytest.mark.parametrize("call", ["dot", "v2"])
@pytest.mark.parametrize("H,D", SHAPES)
def test_a_sequential_fp32_emulation_stays_inside_the_bound(call, H, D):
    ops, ef = case_operands(call, H, D), edge_rows(H, D)
    ref, L, S = edge_ref(call, PTR, IDX, ops, H, ef)
    plain = full_ref(call, PTR, IDX, ops, H)
    assert np.isfinite(ref).all() and not np.allclose(ref, plain[0])               # ef is in use
    ratio = worst_ratio(fp32_chain_edge(call, PTR, IDX, ops, H, ef), ref, edge_bound(L, S, H))
    print("fp32 emulation, %s %dx%d with ef: worst ratio %.4f" % (call, H, D, ratio))
    assert 0.0 < ratio <= 1.0
    # and the emulation with ef = 0 is the emulation without it (x + 0 = x)
    if (H, D) in ((1, 8), (4, 3)):
        zero = np.zeros((E, H * D), f32)
        assert np.array_equal(fp32_chain_edge(call, PTR, IDX, ops, H, zero), fp32_chain_bias(call, PTR, IDX, ops, H, np.zeros(E, f32)))


# ------------------------------------------------------------------------------------------------------- declared, exported, typed
I64, P, I, F = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_float
NEW = {
    "gnnagg_gatv2_run_edge": (r"int gnnagg_gatv2_run_edge\(gnnagg_handle h, const void \*d_xs, const void \*d_xd, int x_dtype, const float \*d_a, "
                              r"const void \*d_ef,\s+long long ef_pitch, void \*d_y, int y_dtype, int feat, int heads, float slope, "
                              r"const float \*d_bias, int bias_heads,\s+float \*d_alpha, float \*d_stat\);",
                              [I64, P, P, I, P, P, I64, P, I, I, I, F, P, I, P, P]),
    "gnnagg_dot_attn_run_edge": (r"int gnnagg_dot_attn_run_edge\(gnnagg_handle h, const void \*d_q, long long q_pitch, const void \*d_k, "
                                 r"const void \*d_v, long long kv_pitch,\s+const void \*d_ef, long long ef_pitch, int x_dtype, void \*d_y, "
                                 r"int y_dtype, int feat, int heads, float scale,\s+const float \*d_bias, int bias_heads, float \*d_alpha, "
                                 r"float \*d_stat\);",
                                 [I64, P, I64, P, P, I64, P, I64, I, P, I, I, I, F, P, I, P, P]),
}


def test_header_declares_and_the_library_exports_the_edge_calls():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, (decl, args) in NEW.items():
        assert re.search(decl, text), name
        assert name in exported
        res, got = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and got == args
        assert getattr(gnc.lib(), name).argtypes == args
    for phrase in ("z_jc = xd[r, c] + (xs[j, c] + ef[p, c])", "k'_p = k[j] + ef[p],  v'_p = v[j] + ef[p]", "WITHOUT ef", "no handle state is added",
                   "ef_pitch < feat"):
        assert phrase in text, phrase
    # the kernels: siblings on the shared frame, named for the shared launcher, through the same pair of switches
    csrc = os.path.join(ROOT, "gnn_computing_amd", "csrc")
    for name, functor, kernel, base in (("agg_gatv2.hip", "Gatv2EdgeKernel", "k_gatv2_edge", "Gatv2Args"),
                                        ("agg_dot.hip", "DotEdgeKernel", "k_dot_attn_edge", "DotArgs")):
        src = open(os.path.join(csrc, name)).read()
        assert re.search(r"struct %s \{[^}]*return %s<VEC, GROUP, NF, TX, SEGRED, BIAS, WEIGHTS>;" % (functor, kernel), src)
        assert re.findall(r"return attn_launch_typed<%s, (\d), (\w+)>\(a, g, stream, no_inst\);" % functor, src) == [("8", "__bf16"), ("4", "float")]
        assert re.search(r"struct \w+EdgeArgs : %s \{[^}]*\bef;[^}]*\bef_pitch;" % base, src)
        assert "hipLaunchKernelGGL" not in src and not re.search(r"\bswitch\s*\(", src)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_the_edge_calls_error_out_without_a_gpu():
    L = gnc.lib()
    x, y, w, s = (np.zeros(8, np.float32) for _ in range(4))
    rc = L.gnnagg_dot_attn_run_edge(ctypes.c_int64(0), x.ctypes.data, 8, x.ctypes.data, x.ctypes.data, 8, x.ctypes.data, 8, 0, y.ctypes.data, 0, 8,
                                    1, ctypes.c_float(0.5), None, 1, w.ctypes.data, s.ctypes.data)
    assert rc == _lib.ERR_HIP and b"no HIP device" in L.gnnagg_last_error()
    rc = L.gnnagg_gatv2_run_edge(ctypes.c_int64(0), x.ctypes.data, x.ctypes.data, 0, x.ctypes.data, x.ctypes.data, 8, y.ctypes.data, 0, 8, 1,
                                 ctypes.c_float(0.2), None, 1, None, None)
    assert rc == _lib.ERR_HIP and b"no HIP device" in L.gnnagg_last_error()
    assert np.all(y == 0) and np.all(w == 0) and np.all(s == 0)


# --------------------------------------------------------------------------------------------------------------- Python-side refusals
def test_edge_is_checked_before_the_library_is_reached(monkeypatch):
    agg, reached = _stub_aggregator(monkeypatch)
    H, n_e, n_v, F_ = 2, agg.num_e, agg.num_v, 8
    x, a = torch.zeros((4, F_)), torch.zeros(F_)
    runs = {"gnnagg_dot_attn_run": [lambda **kw: agg.run_dot(x, x, x, x.clone(), heads=H, **kw), lambda **kw: gnc.dot_attn_run(agg, x, x, x, x.clone(), heads=H, **kw)],
            "gnnagg_gatv2_run": [lambda **kw: agg.run_v2(x, x, a, x.clone(), heads=H, **kw), lambda **kw: gnc.gatv2_run(agg, x, x, a, x.clone(), heads=H, **kw)]}
    where = {"gnnagg_dot_attn_run": 6, "gnnagg_gatv2_run": 5}         # the position of d_ef among the arguments; ef_pitch follows
    ok = torch.zeros((n_e, F_))
    for old, forms in runs.items():
        for run in forms:
            # a wrong dtype (the operands are float32), and things that are no tensor
            for bad in (np.zeros((n_e, F_), np.float32), [[0.0] * F_] * n_e, 0.0, torch.zeros((n_e, F_), dtype=torch.float64),
                        torch.zeros((n_e, F_), dtype=torch.bfloat16), torch.zeros((n_e, F_), dtype=torch.int32)):
                with pytest.raises(TypeError, match="edge"):
                    run(edge=bad)
            # the wrong number of rows, of columns, of dimensions
            for bad in (torch.zeros((n_e + 1, F_)), torch.zeros((n_e - 1, F_)), torch.zeros((n_e, F_ + 1)), torch.zeros((n_e, F_ // H)),
                        torch.zeros((F_, n_e)), torch.zeros(n_e * F_), torch.zeros((n_e, F_, 1)), torch.zeros((n_e, H, F_ // H)), torch.zeros(())):
                with pytest.raises(ValueError, match="edge must be"):
                    run(edge=bad)
            # stride(1) != 1
            for bad in (torch.zeros((F_, n_e)).t(), torch.zeros((n_e, 2 * F_))[:, ::2]):
                assert tuple(bad.shape) == (n_e, F_) and bad.stride(1) != 1
                with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
                    run(edge=bad)
            # a pitch below F (overlapping rows)
            for pitch in (F_ - 1, 1, 0):
                bad = torch.zeros(n_e * F_).as_strided((n_e, F_), (pitch, 1))
                with pytest.raises(ValueError, match="row pitch"):
                    run(edge=bad)
            # a bad bias, bad weights are still refused with edge given
            with pytest.raises(ValueError, match="bias must be"):
                run(edge=ok, bias=torch.zeros(n_e + 1))
            with pytest.raises(ValueError, match="stats without weights"):
                run(edge=ok, stats=torch.zeros((n_v, H, 2)))
            assert reached == []          # neither the stream nor the library
            # None: today's entry points
            with pytest.raises(_NoDevice):
                run()
            with pytest.raises(_NoDevice):
                run(edge=None)
            with pytest.raises(_NoDevice):
                run(edge=None, bias=torch.zeros(n_e))
            with pytest.raises(_NoDevice):
                run(edge=None, weights=torch.zeros((n_e, H)))
            assert [n for n, _ in reached] == ["stream", old, "stream", old, "stream", old + "_bias", "stream", old + "_weights"]
            del reached[:]
            # a valid edge: ONE call of the new entry point, with the pointer, the pitch, and bias and weights passed through
            wide = torch.zeros((n_e, 3 * F_))
            w_ok, s_ok = torch.zeros((n_e, H)), torch.zeros((n_v, H, 2))
            for good, pitch in ((ok, F_), (wide[:, F_:2 * F_], 3 * F_), (torch.zeros(n_e * F_ + 3)[3:].view(n_e, F_), F_),
                                (torch.zeros(n_e * (F_ + 1)).as_strided((n_e, F_), (F_ + 1, 1)), F_ + 1)):
                for bias, bh in ((None, 1), (torch.zeros(n_e), 1), (torch.zeros((n_e, H)), H)):
                    for weights, stats in ((None, None), (w_ok, s_ok), (w_ok, None)):
                        with pytest.raises(_NoDevice):
                            run(edge=good, bias=bias, weights=weights, stats=stats)
                        (s, _), (name, args) = reached
                        assert s == "stream" and name == old + "_edge"
                        assert args[where[old]].value == good.data_ptr() and args[where[old] + 1] == pitch
                        assert args[-3] == bh and ((args[-4] is None) if bias is None else (args[-4].value == bias.data_ptr()))
                        if weights is None:
                            assert args[-2] is None and args[-1] is None
                        else:
                            assert args[-2].value == w_ok.data_ptr() and args[-1].value not in (None, 0)
                            assert stats is None or args[-1].value == s_ok.data_ptr()
                        del reached[:]
    # the device: an edge tensor on the CPU with operands elsewhere
    xm, am = torch.zeros((4, F_), device="meta"), torch.zeros(F_, device="meta")
    for run in (lambda **kw: agg.run_dot(xm, xm, xm, torch.zeros((4, F_), device="meta"), heads=H, **kw),
                lambda **kw: agg.run_v2(xm, xm, am, torch.zeros((4, F_), device="meta"), heads=H, **kw)):
        with pytest.raises(ValueError, match="edge is on cpu, the operands on meta"):
            run(edge=ok)
    assert reached == []
    # bf16 operands want a bf16 edge
    xb = torch.zeros((4, F_), dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="edge must have the operands' dtype"):
        agg.run_dot(xb, xb, xb, xb.clone(), heads=H, edge=ok)
    with pytest.raises(_NoDevice):
        agg.run_v2(xb, xb, a, xb.clone(), heads=H, edge=ok.to(torch.bfloat16))
    assert reached[-1][0] == "gnnagg_gatv2_run_edge"


# --------------------------------------------------------------------------------------------------------------- the example
@pytest.mark.parametrize("model", ["our_GCN", "our_GAT"])
def test_the_example_refuses_edge_dim_with_the_models_without_attention_operands(model):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "forward_3layer.py"), "--model", model, "--edge-dim", "16"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"--edge-dim needs" in r.stderr and r.stdout == b""


def test_the_example_model_takes_edge_dim_last():
    import inspect
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import forward_3layer as f3
    params = list(inspect.signature(f3.Model.__init__).parameters.values())
    assert params[-1].name == "edge_dim" and params[-1].default == 0
    for fn in (gnc.Aggregator_GAT.run_v2, gnc.Aggregator_GAT.run_dot, gnc.gatv2_run, gnc.dot_attn_run):
        names = list(inspect.signature(fn).parameters)
        assert names[-1] == "edge" and names[-2] == "stats" and inspect.signature(fn).parameters["edge"].default is None
