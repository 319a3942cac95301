"""GPU: the per-edge feature vectors of the two online-softmax attention calls -- gnnagg_gatv2_run_edge (Aggregator_GAT.run_v2(edge=)) and
gnnagg_dot_attn_run_edge (Aggregator_GAT.run_dot(edge=)): a row ef[p] of F elements per edge position, added to the gathered row where it
is scored (both calls) and where it is summed (the dot-product only) (include/gnnagg.h).  Judges, inputs and the bound are pinned on the CPU
in tests/test_attn_edge_host.py.

The anchor is the EXPANDED GRAPH: with xs' = xs[idx] + ef (k', v' for the dot-product; one fp32 torch add) and idx' = arange(E) the row
lengths and the lane geometry are the same, so for fp32 operands run_dot(edge=ef) on (ptr, idx) is run_dot(q, k', v') on (ptr, idx') bit
for bit -- y, alpha and stats -- and run_v2(edge=ef) has that graph's alpha and stats (its y sums xs[j], and is judged by the bound).

  1. the identity over every lane geometry of geometry_census.GATV2; bf16 operands against the float64 judge;
  2. ef of all +0.0 is the call without edge, element for element;
  3. bias forms and weights-out with edge: the identity (fp32), the bound (bf16), -Inf bias patterns;
  4. non-finite ef elements: the class map of the judge; every (row, head) they do not reach keeps its bits;
  5. an unaligned ef (element offset 1, pitch F + 1, a column view) gives the aligned bits;
  6. one handle for edge and non-edge calls of both kinds; 7. HIP-graph capture; 8. the refusals of the C-ABI;
  9. the 3-layer forwards of examples/forward_3layer.py with --edge-dim."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import geometry_census
import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_attn_bias_host import DEG, E, IDX, N_SRC, PTR, V, case_operands, head_of, random_bias
from test_attn_edge_host import ARANGE, dot_attn_edge_ref, edge_bound, edge_ref, edge_rows, gatv2_edge_ref
from test_attn_nonfinite_host import PATTERNS, SCORED, SEG, SHAPES, SLOPE, attn_operands, bf16_exact, mask_edges, pattern_id
from test_gatv2_host import worst_ratio
from test_gpu_attn_nonfinite import np_of, on_device, same_bits
from test_gpu_bf16_gat import DEV, dev
from test_gpu_gatv2 import full
from test_nonfinite_host import assert_same_classes

pytestmark = pytest.mark.gpu

F32, B16 = torch.float32, torch.bfloat16
CALLS = ("dot", "v2")
EMPTY = DEG == 0
ROWS = np.repeat(np.arange(V), DEG)
NINF = -np.inf
LONGEST = int(np.argmax(DEG))


def launch(call, agg, t, H, y, edge=None, bias=None, weights=None, stats=None):
    if call == "dot":
        return agg.run_dot(t["q"], t["k"], t["v"], y, heads=H, bias=bias, weights=weights, stats=stats, edge=edge)
    return agg.run_v2(t["xs"], t["xd"], t["a"], y, heads=H, slope=SLOPE, bias=bias, weights=weights, stats=stats, edge=edge)


def handles(F):
    """the aggregator of the graph and the one of the expanded graph (ptr, arange(E))"""
    return gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F), gnc.Aggregator_GAT(dev(PTR), dev(ARANGE), F, F)


def expand(call, t, didx, ef):
    """the operands of the expanded graph: every edge's own source row, ONE fp32 torch add per element"""
    out = dict(t)
    for name in (("k", "v") if call == "dot" else ("xs",)):
        out[name] = t[name][didx] + ef
        assert out[name].dtype == ef.dtype and out[name].shape == ef.shape
    return out


def run_all(call, agg, t, H, edge=None, bias=None, ydt=F32):
    """(y, alpha, stats) of the weights-out call as numpy, after checking that the call without weights gives the same y"""
    F = t[SCORED[call]].shape[1]
    y, y2 = full((V, F), ydt), full((V, F), ydt)
    w, s = full((E, H)), full((V, H, 2))
    assert launch(call, agg, t, H, y, edge, bias, w, s) is s
    assert launch(call, agg, t, H, y2, edge, bias) is None
    assert same_bits(np_of(y), np_of(y2)), "the weights-out call changes y"
    return np_of(y), np_of(w), np_of(s)


def run_y(call, agg, t, H, edge, bias=None, what=""):
    """the fp32 y of one run as numpy, after checking that the bf16 y of the same run is one rounding of it and that rows without edges
    are +0 (the way tests/test_gpu_dot_attn.py judges a bf16 y)"""
    F = t[SCORED[call]].shape[1]
    y32, y16 = full((V, F)), full((V, F), B16)
    launch(call, agg, t, H, y32, edge, bias)
    launch(call, agg, t, H, y16, edge, bias)
    assert same_bits(np_of(y16), np_of(y32.to(B16))), "%s: the bf16 y is not one rounding of the fp32 y" % what
    y = y32.cpu().numpy()
    assert np.all(y[EMPTY] == 0) and not np.signbit(y[EMPTY]).any(), "%s: a row without edges is not +0" % what
    return y


def tag(call, H, D, dt, extra=""):
    return "%s %dx%d %s x%s" % (call, H, D, "bf16" if dt == B16 else "fp32", extra and ", " + extra)


def assert_identity(call, got, want, what):
    """fp32: the edge call against the plain call on the expanded graph -- the dot-product in y, alpha and stats; GATv2 in alpha and stats"""
    names = ("y", "alpha", "stats") if call == "dot" else ("alpha", "stats")
    for name, a, b in zip(("y", "alpha", "stats"), got, want):
        if name in names:
            assert same_bits(a, b), "%s: %s differs from the plain call on the expanded graph" % (what, name)


# ------------------------------------------------------------------------------------------ 1. the identity, every lane geometry
@pytest.mark.parametrize("H,D", sorted(geometry_census.GATV2))
def test_the_edge_call_is_the_plain_call_on_the_expanded_graph(H, D):
    F = H * D
    agg, aggx = handles(F)
    didx = dev(IDX).long()
    ef_np = edge_rows(H, D)
    for call in CALLS:
        ops = case_operands(call, H, D)
        ref, L, S = edge_ref(call, PTR, IDX, ops, H, ef_np)
        bound = edge_bound(L, S, H)
        assert np.isfinite(ref).all()
        # fp32 operands: bit for bit
        t, ef = on_device(call, ops, F32), dev(ef_np)
        got = run_all(call, agg, t, H, edge=ef)
        want = run_all(call, aggx, expand(call, t, didx, ef), H)
        assert_identity(call, got, want, tag(call, H, D, F32))
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        plain = full((V, F))
        launch(call, agg, t, H, plain)
        assert not torch.equal(plain, dev(got[0]))                                  # ef is in use
        # both operand types: the float64 judge on the (widened) inputs
        for dt in (F32, B16):
            what = tag(call, H, D, dt)
            y = run_y(call, agg, on_device(call, ops, dt), H, dev(ef_np).to(dt), what=what)
            ratio = worst_ratio(y, ref, bound)
            print("%s: worst |y - ref| / bound = %.4f" % (what, ratio))
            assert np.isfinite(y).all() and ratio <= 1.0, "%s: worst ratio %.3g against the bound" % (what, ratio)
            if dt == F32:
                assert same_bits(y, got[0])


# ------------------------------------------------------------------------------------------ 2. ef of all +0.0
@pytest.mark.parametrize("H,D", SHAPES)
def test_zero_edge_rows_give_the_values_of_the_call_without_them(H, D):
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    for call in CALLS:
        ops = case_operands(call, H, D)
        for dt in (F32, B16):
            t = on_device(call, ops, dt)
            zero = torch.zeros((E, F), device=DEV, dtype=dt)
            for ydt in (F32, B16):
                want, got = run_all(call, agg, t, H, ydt=ydt), run_all(call, agg, t, H, edge=zero, ydt=ydt)
                for name, a, b in zip(("y", "alpha", "stats"), got, want):
                    # == on every element (only the sign of a zero may differ); nothing here is NaN
                    assert np.array_equal(a, b), "%s: a +0.0 ef changes %s" % (tag(call, H, D, dt), name)
                assert np.isfinite(got[0]).all()


# ------------------------------------------------------------------------------------------ 3. with bias and weights
def bias_forms(H):
    return (("none", None), ("[E]", random_bias(H, False)), ("[E, H]", random_bias(H, True)))


@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (4, 3), (2, 301)])
def test_bias_and_weights_with_edge_rows(H, D):
    F = H * D
    agg, aggx = handles(F)
    didx = dev(IDX).long()
    ef_np = edge_rows(H, D)
    for call in CALLS:
        ops = case_operands(call, H, D)
        t, ef = on_device(call, ops, F32), dev(ef_np)
        tx = expand(call, t, didx, ef)
        for form, bias in bias_forms(H):
            db = None if bias is None else dev(bias)
            # fp32: the identity with the same bias, with weights (run_all) and without (it checks that y is the same)
            got, want = run_all(call, agg, t, H, edge=ef, bias=db), run_all(call, aggx, tx, H, bias=db)
            assert_identity(call, got, want, tag(call, H, D, F32, "bias " + form))
            # bf16 (and GATv2's fp32 y): the bound, L widened by |bias|
            ref, L, S = edge_ref(call, PTR, IDX, ops, H, ef_np, bias)
            bound = edge_bound(L, S, H)
            for dt in (F32, B16):
                what = tag(call, H, D, dt, "bias " + form)
                y = run_y(call, agg, on_device(call, ops, dt), H, dev(ef_np).to(dt), db, what)
                ratio = worst_ratio(y, ref, bound)
                print("%s: worst |y - ref| / bound = %.4f" % (what, ratio))
                assert np.isfinite(y).all() and ratio <= 1.0, "%s: worst ratio %.3g against the bound" % (what, ratio)


@pytest.mark.parametrize("pattern", [("first", 1), ("segment", "middle"), "all"], ids=pattern_id)
@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (4, 3), (2, 301)])
def test_a_bias_mask_masks_as_in_the_plain_call(H, D, pattern):
    assert pattern in PATTERNS
    F, h = H * D, head_of(H)
    mask = mask_edges(PTR, pattern)
    gone = (DEG > 0) & (np.add.reduceat(np.append(~mask, False).astype(np.int64), PTR[:-1]) * (DEG > 0) == 0)      # rows masked whole
    assert (pattern == "all") == bool(gone[DEG > 0].all())
    agg, aggx = handles(F)
    didx = dev(IDX).long()
    ef_np = edge_rows(H, D)
    for call in CALLS:
        ops = case_operands(call, H, D)
        t, ef = on_device(call, ops, F32), dev(ef_np)
        tx = expand(call, t, didx, ef)
        for per_head in (True, False):
            bias = random_bias(H, per_head).copy()
            if per_head:
                bias[mask, h] = NINF
            else:
                bias[mask] = NINF
            what = tag(call, H, D, F32, "%s, bias %s" % (pattern_id(pattern), "[E, H]" if per_head else "[E]"))
            got, want = run_all(call, agg, t, H, edge=ef, bias=dev(bias)), run_all(call, aggx, tx, H, bias=dev(bias))
            assert_identity(call, got, want, what)
            with np.errstate(all="ignore"):
                ref, _, _ = edge_ref(call, PTR, IDX, ops, H, ef_np, bias)
            assert_same_classes(got[0], ref, what)
            # a masked edge weighs exactly +0 -- or NaN where its whole (row, head) is masked
            alpha = got[1][:, [h] if per_head else slice(None)]
            assert (alpha[mask & ~gone[ROWS]] == 0).all() and np.isnan(alpha[gone[ROWS]]).all() and np.isfinite(alpha[~gone[ROWS]]).all()
            hit = slice(h * D, (h + 1) * D) if per_head else slice(None)
            assert np.isnan(got[0][gone][:, hit]).all() and np.isnan(ref[gone][:, hit]).all() and np.isfinite(got[0][~gone]).all()


# ------------------------------------------------------------------------------------------ 4. non-finite ef
@pytest.mark.parametrize("bad", [-np.inf, np.inf, np.nan], ids=["ninf", "inf", "nan"])
@pytest.mark.parametrize("H,D", [(1, 8), (8, 16), (4, 3), (2, 301)])
def test_a_non_finite_edge_element_reaches_its_row_and_head_only(H, D, bad):
    F, h = H * D, head_of(H)
    n = int(DEG[LONGEST])
    assert n > 3 * SEG
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    ef_np = edge_rows(H, D)
    b, e = int(PTR[LONGEST]), int(PTR[LONGEST + 1])
    sub_ptr, sub_idx = np.array([0, n]), IDX[b:e]
    cols = np.zeros(F, bool)
    cols[h * D:(h + 1) * D] = True
    for where, p in (("early", 1), ("middle segment", SEG + SEG // 2), ("last", n - 1)):
        ef_bad = ef_np.copy()
        ef_bad[b + p, h * D] = bad                       # the masking column of head h (attn_operands: q, a positive there)
        for call in CALLS:
            ops = case_operands(call, H, D)
            sub = dict(ops)
            sub["q" if call == "dot" else "xd"] = ops["q" if call == "dot" else "xd"][LONGEST:LONGEST + 1]
            with np.errstate(all="ignore"):
                ref, _, _ = edge_ref(call, sub_ptr, sub_idx, sub, H, ef_bad[b:e])
            assert not np.isfinite(ref).all() or (call == "v2" and bad == -np.inf)
            for dt in (F32, B16):
                what = tag(call, H, D, dt, "%r in the %s edge" % (bad, where))
                t = on_device(call, ops, dt)
                clean = run_all(call, agg, t, H, edge=dev(ef_np).to(dt))
                got = run_all(call, agg, t, H, edge=dev(ef_bad).to(dt))
                assert np.isfinite(clean[0]).all()
                assert_same_classes(got[0][LONGEST:LONGEST + 1], ref, what)
                # every (row, head) the value does not reach: the bits of the run without it -- y, alpha and stats
                other = np.ones((V, F), bool)
                other[LONGEST, cols] = False
                assert same_bits(got[0][other], clean[0][other]), "%s: y of another (row, head) differs" % what
                eh = np.ones((E, H), bool)
                eh[b:e, h] = False
                assert same_bits(got[1][eh], clean[1][eh]), "%s: alpha of another (row, head) differs" % what
                rh = np.ones((V, H), bool)
                rh[LONGEST, h] = False
                assert same_bits(got[2][rh], clean[2][rh]), "%s: stats of another (row, head) differ" % what
                if bad == -np.inf:
                    assert got[1][b + p, h] == 0 and not np.signbit(got[1][b + p, h])              # masked: a weight of exactly +0
                else:
                    assert np.isnan(got[0][LONGEST, cols]).all() and np.isnan(got[1][b:e, h]).all()


# ------------------------------------------------------------------------------------------ 5. an unaligned ef
@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,D", [(8, 16), (2, 301)])
def test_an_unaligned_ef_gives_the_bits_of_an_aligned_one(H, D, dt):
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    ef = dev(edge_rows(H, D)).to(dt)
    assert ef.data_ptr() % 16 == 0 and ef.is_contiguous()
    esize = ef.element_size()
    # element offset 1; a pitch of F + 1; a column view of a wider tensor (offset F + 1, pitch 3 F + 2)
    shifted = torch.full((E * F + 8,), float("nan"), device=DEV, dtype=dt)[1:1 + E * F].view(E, F)
    pitched = torch.full((E, F + 1), float("nan"), device=DEV, dtype=dt)[:, :F]
    column = torch.full((E, 3 * F + 2), float("nan"), device=DEV, dtype=dt)[:, F + 1:2 * F + 1]
    for view in (shifted, pitched, column):
        view.copy_(ef)
    assert shifted.data_ptr() % 16 == esize and shifted.stride(0) == F
    assert pitched.stride(0) == F + 1 and column.stride(0) == 3 * F + 2 and column.data_ptr() % 16 != 0
    for call in CALLS:
        t = on_device(call, case_operands(call, H, D), dt)
        want = run_all(call, agg, t, H, edge=ef)
        assert np.isfinite(want[0]).all()
        for name, view in (("offset 1", shifted), ("pitch F + 1", pitched), ("column view", column)):
            got = run_all(call, agg, t, H, edge=view)
            for part, a, b in zip(("y", "alpha", "stats"), got, want):
                assert same_bits(a, b), "%s: ef at %s changes the bits of %s" % (tag(call, H, D, dt), name, part)


# ------------------------------------------------------------------------------------------ 6. one handle
def test_a_handle_serving_edge_and_plain_calls_of_both_kinds():
    """no handle state is added: call by call the bits of a fresh handle"""
    dptr, didx = dev(PTR), dev(IDX)
    # (call, H, D, x dtype, y dtype, bias: None / "heads" / "one", edge, weights)
    calls = [("dot", 4, 8, B16, F32, "heads", True, False), ("v2", 1, 8, F32, F32, None, False, True), ("dot", 1, 602, F32, B16, "one", True, True),
             ("v2", 8, 16, B16, B16, "heads", True, True), ("dot", 8, 16, F32, F32, None, True, False), ("v2", 2, 301, F32, F32, "one", True, False),
             ("dot", 8, 32, F32, F32, "heads", False, False), ("v2", 8, 16, B16, B16, None, True, False), ("dot", 4, 8, B16, F32, None, False, True),
             ("v2", 1, 8, F32, F32, "heads", True, True), ("dot", 1, 1000, F32, F32, None, True, True), ("v2", 4, 128, F32, B16, None, True, False)]

    def one(agg, n, call, H, D, xdt, ydt, kind, edge, weights):
        ops = attn_operands(call, V, N_SRC, H, D, head_of(H), seed=900 + n)
        bias = None if kind is None else dev(random_bias(H, kind == "heads"))
        ef = dev(edge_rows(H, D)).to(xdt) if edge else None
        y, w = full((V, H * D), ydt), full((E, H))
        s = launch(call, agg, on_device(call, ops, xdt), H, y, ef, bias, w if weights else None)
        return (y, w, s) if weights else (y,)
    for first in (0, 1):
        shared = gnc.Aggregator_GAT(dptr, didx, 8, 8)
        for n, c in enumerate(calls[first:]):
            got = one(shared, n, *c)
            want = one(gnc.Aggregator_GAT(dptr, didx, c[1] * c[2], c[1] * c[2]), n, *c)
            for a, b in zip(got, want):
                assert torch.equal(a, b), "call %d %r on the shared handle differs from a fresh one" % (n, c)
            assert torch.isfinite(got[0].float()).all()


# ------------------------------------------------------------------------------------------ 7. capture and replay
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (2, 301)])
def test_graph_capture_and_replay_of_an_edge_call(call, H, D):
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    t = on_device(call, case_operands(call, H, D), B16)
    ef = dev(edge_rows(H, D)).to(B16).clone()
    bias = dev(random_bias(H, True))
    for ydt in (F32, B16):
        y, w, s = full((V, F), ydt), full((E, H)), full((V, H, 2))
        launch(call, agg, t, H, y, ef, bias, w, s)          # warm call: the list of long rows, the scratch
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                           # (captures on a side stream: the call may neither allocate nor synchronise)
            launch(call, agg, t, H, y, ef, bias, w, s)
        first = None
        for seed in (53, 54):
            ef.copy_(dev(bf16_exact(np.random.default_rng(seed).standard_normal((E, F)))).to(B16))      # rewritten in place
            y.fill_(7.0), w.fill_(7.0), s.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            ey, ew, es = full((V, F), ydt), full((E, H)), full((V, H, 2))
            launch(call, agg, t, H, ey, ef, bias, ew, es)
            assert same_bits(np_of(y), np_of(ey)) and same_bits(np_of(w), np_of(ew)) and same_bits(np_of(s), np_of(es))
            assert torch.isfinite(y.float()).all()
            assert first is None or not torch.equal(first, y)                                        # the new ef is honoured
            first = y.clone()


# ------------------------------------------------------------------------------------------ 8. the C-ABI
def test_cabi_refusals_of_the_edge_calls_leave_the_outputs_alone():
    F = 16
    dptr, didx = dev(PTR), dev(IDX)
    gat = gnc.Aggregator_GAT(dptr, didx, F, F)
    gcn = gnc.Aggregator_GCN(dptr, didx, None, F, F)
    big = gnc.Aggregator_GAT.GATV2_MAX_FEAT + 8
    x, a, y, b = torch.zeros((N_SRC, big), device=DEV), torch.zeros(big, device=DEV), full((V, big)), torch.zeros((E, 8), device=DEV)
    ef, w, s = torch.zeros((E, big), device=DEV), full((E, 8)), full((V, 8, 2))
    L = gnc.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def dot(text, h=None, q=x, k=x, v=x, qp=big, kvp=big, e=ef, ep=big, xt=0, yv=y, yt=0, feat=F, heads=2, scale=0.5, bias=b, bh=2, wv=w, sv=s,
            rc_want=_lib.ERR_ARG):
        rc = L.gnnagg_dot_attn_run_edge(gat._h if h is None else h, p(q), qp, p(k), p(v), kvp, p(e), ep, xt, p(yv), yt, feat, heads,
                                        ctypes.c_float(scale), p(bias), bh, p(wv), p(sv))
        err = L.gnnagg_last_error()
        assert rc == rc_want and (rc == 0 or (b"gnnagg_dot_attn_run_edge:" in err and text in err)), err

    def v2(text, h=None, xs=x, xd=x, xt=0, av=a, e=ef, ep=big, yv=y, yt=0, feat=F, heads=2, slope=0.2, bias=b, bh=2, wv=w, sv=s,
           rc_want=_lib.ERR_ARG):
        rc = L.gnnagg_gatv2_run_edge(gat._h if h is None else h, p(xs), p(xd), xt, p(av), p(e), ep, p(yv), yt, feat, heads,
                                     ctypes.c_float(slope), p(bias), bh, p(wv), p(sv))
        err = L.gnnagg_last_error()
        assert rc == rc_want and (rc == 0 or (b"gnnagg_gatv2_run_edge:" in err and text in err)), err
    for f in (dot, v2):
        # the refusals of the _weights calls, under these names
        f(b"not a GAT aggregator", h=gcn._h)
        f(b"d_y", yv=None)
        f(b"x_dtype 7", xt=7)
        f(b"y_dtype -1", yt=-1)
        f(b"feat = 0", feat=0)
        f(b"heads = 3", heads=3)
        f(("limit of %d" % gnc.Aggregator_GAT.GATV2_MAX_FEAT).encode(), feat=big, heads=1, bh=1)
        for n in (0, 3, -1, 16):
            f(("bias_heads = %d" % n).encode(), bh=n)
        # ... and the call's own
        f(b"d_ef", e=None)
        f(b"ef_pitch = 15", ep=15)
        f(b"ef_pitch = -16", ep=-16)
        f(b"ef_pitch = 0", ep=0)
        f(b"d_alpha", wv=None)
        f(b"d_stat", sv=None)
    dot(b"d_q", q=None)
    dot(b"d_k", k=None)
    dot(b"d_v", v=None)
    dot(b"q_pitch = 15", qp=15)
    dot(b"scale", scale=float("nan"))
    v2(b"d_xs", xs=None)
    v2(b"d_xd", xd=None)
    v2(b"d_a", av=None)
    v2(b"slope", slope=1.5)
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (w == 7.0).all() and (s == 7.0).all()
    # what is accepted: no bias (bias_heads ignored), no weights (both null), and both together -- the bits of the Python calls
    xs, av, e16 = torch.randn((N_SRC, F), device=DEV), torch.randn(F, device=DEV), torch.randn((E, F), device=DEV)
    for f, call, t in ((dot, "dot", dict(q=xs, k=xs, v=xs)), (v2, "v2", dict(xs=xs, xd=xs, a=av))):
        kw = dict(q=xs, k=xs, v=xs, qp=F, kvp=F, scale=0.5) if call == "dot" else dict(xs=xs, xd=xs, av=av, slope=SLOPE)
        for bias, bh in ((None, 99), (b[:, :2].contiguous(), 2), (b[:, :1].contiguous(), 1)):
            for weights in (False, True):
                yy, ww, ss = full((V, F)), full((E, 2)), full((V, 2, 2))
                f(b"", e=e16, ep=F, yv=yy, bias=bias, bh=bh, wv=ww if weights else None, sv=ss if weights else None, rc_want=0, **kw)
                wy, wwant, swant = full((V, F)), full((E, 2)), full((V, 2, 2))
                if call == "dot":
                    gat.run_dot(xs, xs, xs, wy, heads=2, scale=0.5, bias=bias, weights=wwant if weights else None, stats=swant if weights else None, edge=e16)
                else:
                    gat.run_v2(xs, xs, av, wy, heads=2, bias=bias, weights=wwant if weights else None, stats=swant if weights else None, edge=e16)
                assert torch.equal(yy, wy) and torch.equal(ww, wwant) and torch.equal(ss, swant) and torch.isfinite(yy).all()
                assert weights or ((ww == 7.0).all() and (ss == 7.0).all())
    # a graph without edges reads no ef: any d_ef is accepted, and the result is all +0
    n_v = 5
    none = gnc.Aggregator_GAT(torch.zeros(n_v + 1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), F, F)
    for e in (None, e16):
        for f, kw in ((dot, dict(q=xs, k=xs, v=xs, qp=F, kvp=F)), (v2, dict(xs=xs, xd=xs, av=av))):
            yy, ss = full((n_v, F)), full((n_v, 2, 2))
            f(b"", h=none._h, e=e, ep=F, yv=yy, bias=None, wv=ss, sv=ss, rc_want=0, **kw)
            assert (yy == 0).all() and not torch.signbit(yy).any()
            assert torch.isneginf(ss[:, :, 0]).all() and (ss[:, :, 1] == 0).all()
    yy = full((n_v, F))
    none.run_dot(xs, xs, xs, yy, heads=2, edge=torch.zeros((0, F), device=DEV))
    assert (yy == 0).all()
    # the Python side refuses before the library
    with pytest.raises(ValueError, match="edge must be"):
        gat.run_dot(xs, xs, xs, full((V, F)), heads=2, edge=torch.zeros((E, F + 1), device=DEV))
    with pytest.raises(ValueError, match="operands on"):
        gat.run_v2(xs, xs, av, full((V, F)), heads=2, edge=torch.zeros((E, F)))


# ------------------------------------------------------------------------------------------ 9. the --edge-dim forwards
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import forward_3layer as f3  # noqa: E402


@pytest.mark.parametrize("model_name", ["our_Transformer", "our_GATv2"])
@pytest.mark.parametrize("dtype,heads", [(torch.float32, 1), (torch.float32, 8), (B16, 8)])
def test_edge_dim_forward_layer_by_layer(model_name, dtype, heads):
    n_v = 2000
    ptr_t, idx_t = gnc.graph.powerlaw_csr(n_v, 30000, seed=123)
    ptr, idx = ptr_t.numpy(), idx_t.numpy()
    n_e = len(idx)
    kw = dict(transformer=True) if model_name == "our_Transformer" else dict(gatv2=True)
    m = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN, dtype=dtype, heads=heads, edge_dim=16, **kw)
    plain = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN, dtype=dtype, heads=heads, **kw)
    assert plain.edge_attr is None and torch.equal(plain.h, m.h) and all(torch.equal(a, b) for a, b in zip(plain.weights, m.weights))
    assert m.edge_attr.shape == (n_e, 16) and m.edge_attr.dtype == dtype and [tuple(w.shape) for w in m.w_edge] == [(16, n) for n in f3.DIMS[1:]]
    with pytest.raises(ValueError, match="edge_dim belongs"):
        f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN, edge_dim=16)
    m.trace = []
    y = m.forward(model_name)
    assert len(m.trace) == 3 and y.shape == (n_v, 32) and y.dtype == dtype and bool(torch.isfinite(y.float()).all())
    assert not torch.equal(y, plain.forward(model_name))
    for k, t in enumerate(m.trace):
        N = f3.DIMS[k + 1]
        ef = t["ef"]
        assert ef.shape == (n_e, N) and ef.dtype == dtype and torch.equal(ef, gnc.matmul_NN(m.edge_attr, m.w_edge[k]))
        ef_np = ef.float().cpu().numpy()
        out32 = torch.full((n_v, N), 7.0, device=DEV)
        if model_name == "our_Transformer":
            q, kk, v = t["qkv"][:, :N], t["qkv"][:, N:2 * N], t["qkv"][:, 2 * N:]
            m.at_gat.run_dot(q, kk, v, out32, heads=heads, edge=ef)
            x = t["qkv"].float().cpu().numpy()
            ref, L, S = dot_attn_edge_ref(ptr, idx, x[:, :N], x[:, N:2 * N], x[:, 2 * N:], ef_np, heads, np.float32(1.0 / math.sqrt(N // heads)))
        else:
            m.at_gat.run_v2(t["feat2"], t["feat2"], t["a"], out32, heads=heads, edge=ef)
            x = t["feat2"].float().cpu().numpy()
            ref, L, S = gatv2_edge_ref(ptr, idx, x, x, t["a"].cpu().numpy(), ef_np, heads, 0.2)
        assert torch.equal(t["out"], out32.to(dtype)), "layer %d: the traced output is not (one rounding of) the fp32 result" % k
        ratio = worst_ratio(out32.cpu().numpy(), ref, edge_bound(L, S, heads))
        print("%s layer %d (%s, %d heads, edge_dim 16): worst |y - ref| / bound = %.4f" % (model_name, k, dtype, heads, ratio))
        assert bool(torch.isfinite(out32).all()) and ratio <= 1.0, "layer %d: worst ratio %.3g" % (k, ratio)
    assert torch.equal(y, m.trace[-1]["out"])


def test_the_example_runs_with_edge_dim_from_the_command_line():
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (one process: the flag's way from the command line into the model, combined with --edge-bias, --heads and bf16; --hip-graph: the
    # script itself asserts that the captured forward replays to the eager bits)
    out = subprocess.check_output([sys.executable, os.path.join(root, "examples", "forward_3layer.py"), "--model", "our_GATv2", "--edge-dim", "16",
                                   "--edge-bias", "--heads", "8", "--dtype", "bf16", "--iters", "1", "--hip-graph"]).decode()
    rec = json.loads(out.strip().splitlines()[-1])
    assert rec["model"] == "our_GATv2" and rec["edge_dim"] == 16 and rec["edge_bias"] is True and rec["finite"] is True and rec["heads"] == 8
