"""GPU: the per-edge score bias of the two online-softmax attention calls -- gnnagg_gatv2_run_bias (Aggregator_GAT.run_v2(bias=)) and
gnnagg_dot_attn_run_bias (Aggregator_GAT.run_dot(bias=)): one fp32 per (edge, head), or per edge, added to the score before the softmax;
-Inf masks the edge (include/gnnagg.h).  Judges, inputs and the conditions on them are pinned on the CPU in tests/test_attn_bias_host.py.

  1. one-hot selection: +0 on one edge per (row, head) and -Inf on every other -- y is that edge's source row, bit for bit: pins the
     addressing of the bias (edge position, head, bias_heads, the offsets of segments and chunks);
  2. a random finite bias against the float64 judge, inside 1e-5 (1 + L) S with L widened by |bias|;
  3. a +0.0 bias is the call without a bias, bit for bit;
  4. masks by position against the graph with the masked edges deleted; the other heads keep their bits; GATv2 has no NaN column;
  5. a +Inf or NaN bias makes exactly its (row, head) NaN;
  6. a constant per (row, head) changes nothing beyond rounding (softmax shift invariance);
  7. one handle for biased and unbiased calls of both kinds, HIP-graph capture, an unaligned bias, the refusals of the C-ABI;
  8. the 3-layer forwards of examples/forward_3layer.py with --edge-bias."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_attn_bias_host import (DEG, E, IDX, N_SRC, PTR, V, bias_bound, bias_ref, biased_spread, case_operands, dot_attn_bias_ref,
                                 gatv2_bias_ref, head_of, random_bias)
from test_attn_nonfinite_host import (PATTERNS, SCORED, SEG, SHAPES, SLOPE, attn_operands, bf16_exact, delete_edges, full_ref, mask_edges,
                                      pattern_id)
from test_dot_attn_host import dot_attn_bound
from test_gatv2_host import gatv2_bound, worst_ratio
from test_gpu_attn_nonfinite import np_of, on_device, same_bits
from test_gpu_bf16_gat import DEV, GRAPHS, dev
from test_gpu_gatv2 import full
from test_nonfinite_host import assert_same_classes

pytestmark = pytest.mark.gpu

F32, B16 = torch.float32, torch.bfloat16
CALLS = ("dot", "v2")
EMPTY = DEG == 0
ROWS = np.repeat(np.arange(V), DEG)
NINF = -np.inf


def launch(call, agg, t, H, y, bias=None):
    if call == "dot":
        agg.run_dot(t["q"], t["k"], t["v"], y, heads=H, bias=bias)
    else:
        agg.run_v2(t["xs"], t["xd"], t["a"], y, heads=H, slope=SLOPE, bias=bias)


def run_y(call, agg, t, H, bias, n_v=V, empty=EMPTY, what=""):
    """the fp32 y of one run (y pre-filled with 7.0) as numpy, after checking that the bf16 y of the same run is one rounding of it and that
    rows without edges are +0"""
    F = t[SCORED[call]].shape[1]
    y32, y16 = full((n_v, F)), full((n_v, F), B16)
    launch(call, agg, t, H, y32, bias)
    launch(call, agg, t, H, y16, bias)
    assert same_bits(np_of(y16), np_of(y32.to(B16))), "%s: the bf16 y is not one rounding of the fp32 y" % what
    y = y32.cpu().numpy()
    assert np.all(y[empty] == 0) and not np.signbit(y[empty]).any(), "%s: a row without edges is not +0" % what
    return y


def tag(call, H, D, dt, extra=""):
    return "%s %dx%d %s x%s" % (call, H, D, "bf16" if dt == B16 else "fp32", extra and ", " + extra)


def summed(call):
    return "v" if call == "dot" else "xs"


# ------------------------------------------------------------------------------------------ 1. one-hot selection, exact
def candidates(n):
    """positions in a row of n edges: the first, the last, a middle one and, for a row of several segments, one in each segment"""
    c = [0, n - 1, n // 2]
    if n > SEG:
        c += [s * SEG + (7 * s + 3) % min(SEG, n - s * SEG) for s in range(-(-n // SEG))]
    return c


N_ROUNDS = max(len(candidates(int(n))) for n in DEG)


def chosen_edges(H, shift):
    """[V, H] edge positions (global; -1 for rows without edges): head h of row r takes candidate (r + h + shift) of its row"""
    pos = np.full((V, H), -1, np.int64)
    for r in np.flatnonzero(DEG > 0):
        c = candidates(int(DEG[r]))
        for h in range(H):
            pos[r, h] = PTR[r] + c[(r + h + shift) % len(c)]
    return pos


def test_the_choices_reach_every_place():
    assert N_ROUNDS == 3 + 4 and (DEG > SEG).sum() >= 3
    hit = [set() for _ in range(V)]
    for shift in range(N_ROUNDS):
        pos = chosen_edges(1, shift)
        for r in np.flatnonzero(DEG > 0):
            hit[r].add(int(pos[r, 0] - PTR[r]))
    for r in np.flatnonzero(DEG > 0):
        n = int(DEG[r])
        assert {0, n - 1, n // 2} <= hit[r]
        if n > SEG:
            assert {p // SEG for p in hit[r]} == set(range(-(-n // SEG)))
    two = chosen_edges(8, 0)
    assert all(len(set(two[r])) > 1 for r in np.flatnonzero(DEG > 2))      # the choice differs between heads


@pytest.mark.parametrize("H,D", SHAPES)
def test_one_hot_bias_selects_one_source_row_exactly(H, D):
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    nz = np.flatnonzero(DEG > 0)
    didx = dev(IDX).long()
    for call in CALLS:
        ops = case_operands(call, H, D)
        for dt in (F32, B16):
            t = on_device(call, ops, dt)
            src = t[summed(call)]
            for shift in range(N_ROUNDS):
                for per_head in (True, False):
                    pos = chosen_edges(H if per_head else 1, shift)
                    bias = np.full((E, H) if per_head else (E,), NINF, np.float32)
                    if per_head:
                        bias[pos[nz], np.arange(H)[None, :]] = 0.0
                    else:
                        bias[pos[nz, 0]] = 0.0
                    dpos = dev(np.where(pos < 0, 0, pos))
                    if not per_head:
                        dpos = dpos.expand(V, H)
                    # expected: columns of head h of row r from the source row of the chosen edge
                    gathered = src[didx[dpos]]                                               # [V, H, F]
                    want = torch.stack([gathered[:, h, h * D:(h + 1) * D] for h in range(H)], dim=1).reshape(V, F).float()
                    want[dev(EMPTY)] = 0.0
                    for ydt in (F32, B16):
                        y = full((V, F), ydt)
                        launch(call, agg, t, H, y, dev(bias))
                        what = tag(call, H, D, dt, "%s y, choice %d, bias %s" % (ydt, shift, "[E, H]" if per_head else "[E]"))
                        assert torch.equal(y, want.to(ydt)), "%s: y is not the chosen edge's source row" % what


# ------------------------------------------------------------------------------------------ 2. random finite bias, the judge
def judge_random_bias(ptr, idx, n_src, H, D, what):
    n_v, n_e, F = len(ptr) - 1, len(idx), H * D
    empty = np.diff(ptr) == 0
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    for call in CALLS:
        ops = attn_operands(call, n_v, n_src, H, D, head_of(H), seed=F)
        for per_head in (True, False):
            bias = random_bias(H, per_head, n_e)
            assert bias.shape == ((n_e, H) if per_head else (n_e,))
            ref, L, S = bias_ref(call, ptr, idx, ops, H, bias, block_edges=max(256, (1 << 22) // F))
            bound = bias_bound(L, S, H)
            for dt in (F32, B16):
                w = tag(call, H, D, dt, "%s, bias %s" % (what, "[E, H]" if per_head else "[E]"))
                y = run_y(call, agg, on_device(call, ops, dt), H, dev(bias), n_v, empty, w)
                ratio = worst_ratio(y, ref, bound)
                print("%s: worst |y - ref| / bound = %.4f" % (w, ratio))
                assert np.isfinite(y).all() and ratio <= 1.0, "%s: worst ratio %.3g against the bound" % (w, ratio)


@pytest.mark.parametrize("H,D", SHAPES)
def test_a_random_finite_bias_is_within_the_bound(H, D):
    judge_random_bias(PTR, IDX, N_SRC, H, D, "thresholds")


@pytest.mark.parametrize("graph", ["uniform", "powerlaw"])
@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (2, 301)])
def test_a_random_finite_bias_on_the_projects_graphs(graph, H, D):
    ptr, idx = GRAPHS[graph]()
    judge_random_bias(np.asarray(ptr), np.asarray(idx), len(ptr) - 1, H, D, graph)


# ------------------------------------------------------------------------------------------ 3. zero bias and null bias
@pytest.mark.parametrize("H,D", SHAPES)
def test_a_zero_bias_gives_the_bits_of_the_call_without_a_bias(H, D):
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    for call in CALLS:
        ops = case_operands(call, H, D)
        for dt in (F32, B16):
            t = on_device(call, ops, dt)
            for ydt in (F32, B16):
                plain, none = full((V, F), ydt), full((V, F), ydt)
                launch(call, agg, t, H, plain)
                launch(call, agg, t, H, none, None)
                assert torch.equal(plain, none) and torch.isfinite(plain.float()).all()
                for zero in (torch.zeros((E, H), device=DEV), torch.zeros(E, device=DEV), torch.zeros((E, 1), device=DEV)):
                    y = full((V, F), ydt)
                    launch(call, agg, t, H, y, zero)
                    assert same_bits(np_of(y), np_of(plain)), "%s: a +0.0 bias %s changes the bits" % (tag(call, H, D, dt), tuple(zero.shape))


# ------------------------------------------------------------------------------------------ 4. masks against the deleted graph
@pytest.mark.parametrize("pattern", PATTERNS, ids=pattern_id)
@pytest.mark.parametrize("H,D", [(1, 8), (8, 16), (4, 3), (2, 301), (8, 128)])
def test_bias_masks_are_weights_of_zero_wherever_they_stand(H, D, pattern):
    F, h = H * D, head_of(H)
    mask = mask_edges(PTR, pattern)
    ptr_d, idx_d = delete_edges(PTR, IDX, mask)
    gone = (DEG > 0) & (np.diff(ptr_d) == 0)
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    for call in CALLS:
        ops = case_operands(call, H, D)
        bound_of = dot_attn_bound if call == "dot" else gatv2_bound
        for per_head in (True, False):
            base = random_bias(H, per_head)
            bias = base.copy()
            if per_head:
                bias[mask, h] = NINF
                heads_hit = [h]
            else:
                bias[mask] = NINF
                heads_hit = list(range(H))
            hit = np.zeros(F, bool)
            for hh in heads_hit:
                hit[hh * D:(hh + 1) * D] = True
            ref_full, _, _ = bias_ref(call, PTR, IDX, ops, H, bias)                 # the class map
            ref_del, L, S = bias_ref(call, ptr_d, idx_d, ops, H, base[~mask])       # the reference and the bound: the masked edges deleted
            bound = bound_of(L, S, H)
            assert np.isfinite(ref_del).all() and np.isnan(ref_full[gone][:, hit]).all() and np.isfinite(ref_full[:, ~hit]).all()
            assert np.array_equal(np.isnan(ref_full), gone[:, None] & hit[None, :])
            # (the deleted graph is the judge of the masked heads only: the other heads keep these edges, and the bits of the unmasked run)
            fin = np.isfinite(ref_full) & hit[None, :]
            for dt in (F32, B16):
                what = tag(call, H, D, dt, "%s, bias %s" % (pattern_id(pattern), "[E, H]" if per_head else "[E]"))
                t = on_device(call, ops, dt)
                y_base = run_y(call, agg, t, H, dev(base), what=what + " (no mask)")
                y = run_y(call, agg, t, H, dev(bias), what=what)
                assert np.isfinite(y_base).all()
                assert_same_classes(y, ref_full, what)
                ratio = worst_ratio(y[fin], ref_del[fin], bound[fin])
                print("%s: worst |y - ref| / bound = %.4f" % (what, ratio))
                assert ratio <= 1.0, "%s: worst ratio %.3g against the bound of the graph with the masked edges deleted" % (what, ratio)
                assert np.isnan(y[gone][:, hit]).all(), "%s: a fully masked (row, head) is not NaN" % what
                assert same_bits(y[:, ~hit], y_base[:, ~hit]), "%s: an untouched head differs from the run without the mask" % what
                if call == "v2":
                    assert not np.isnan(y[~gone]).any(), "%s: a NaN column in a row that keeps an edge" % what


# ------------------------------------------------------------------------------------------ 5. +Inf and NaN biases
@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("H,D", [(1, 8), (8, 16), (4, 3), (2, 301), (8, 128)])
def test_an_inf_or_nan_bias_makes_exactly_its_row_head_nan(H, D, bad):
    F, h = H * D, head_of(H)
    rows = np.union1d(np.flatnonzero(DEG > 0)[::3], [int(np.argmax(DEG))])
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    for where in ("first", "middle", "last"):
        pos = {"first": PTR[:-1], "middle": PTR[:-1] + DEG // 2, "last": PTR[1:] - 1}[where][rows]
        for per_head in (True, False):
            base = random_bias(H, per_head)
            bias = base.copy()
            expect = np.zeros((V, F), bool)
            if per_head:
                bias[pos, h] = bad
                expect[rows, h * D:(h + 1) * D] = True
            else:
                bias[pos] = bad
                expect[rows] = True
            for call in CALLS:
                ops = case_operands(call, H, D)
                for dt in (F32, B16):
                    what = tag(call, H, D, dt, "%r on the %s edge, bias %s" % (bad, where, "[E, H]" if per_head else "[E]"))
                    t = on_device(call, ops, dt)
                    y_base = run_y(call, agg, t, H, dev(base), what=what + " (finite)")
                    y = run_y(call, agg, t, H, dev(bias), what=what)
                    assert np.isfinite(y_base).all()
                    assert np.array_equal(np.isnan(y), expect), "%s: NaN in other places than the (row, head)s of the value" % what
                    assert same_bits(y[~expect], y_base[~expect]), "%s: another (row, head) differs from the run with a finite value" % what


# ------------------------------------------------------------------------------------------ 6. a constant per (row, head)
@pytest.mark.parametrize("H,D", [(1, 8), (8, 16), (4, 3), (2, 301), (8, 128)])
def test_a_constant_per_row_and_head_changes_nothing_beyond_rounding(H, D):
    """softmax is invariant under a shift of a (row, head)'s scores: against the reference WITHOUT a bias, inside the bias judge's bound"""
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    c = bf16_exact(np.random.default_rng(H * D).uniform(-8.0, 8.0, (V, H)))
    assert np.abs(c).max() <= 8.0
    for call in CALLS:
        ops = case_operands(call, H, D)
        ref, L0, S0 = full_ref(call, PTR, IDX, ops, H)
        for per_head in (True, False):
            bias = np.ascontiguousarray(c[ROWS] if per_head else c[ROWS, 0])
            ref_b, L, S = bias_ref(call, PTR, IDX, ops, H, bias)
            bound = bias_bound(L, S, H)
            assert np.all(L >= L0) and (np.abs(ref_b - ref) <= 1e-7 * bound).all()       # the judge itself is shift-invariant
            for dt in (F32, B16):
                what = tag(call, H, D, dt, "constant per row, bias %s" % ("[E, H]" if per_head else "[E]"))
                y = run_y(call, agg, on_device(call, ops, dt), H, dev(bias), what=what)
                ratio = worst_ratio(y, ref, bound)
                print("%s: worst |y - unbiased ref| / bound = %.4f" % (what, ratio))
                assert ratio <= 1.0


# ------------------------------------------------------------------------------------------ 7. plumbing
def test_a_handle_serving_biased_and_unbiased_calls_of_both_kinds():
    """no handle state is added: call by call the bits of a fresh handle"""
    dptr, didx = dev(PTR), dev(IDX)
    # (call, H, D, x dtype, y dtype, bias: None / "heads" / "one")
    calls = [("dot", 4, 8, B16, F32, "heads"), ("v2", 1, 8, F32, F32, None), ("dot", 1, 602, F32, B16, "one"), ("v2", 8, 16, B16, B16, "heads"),
             ("dot", 8, 16, F32, F32, None), ("v2", 2, 301, F32, F32, "one"), ("dot", 8, 32, F32, F32, "heads"), ("v2", 8, 16, B16, B16, None),
             ("dot", 4, 8, B16, F32, None), ("v2", 1, 8, F32, F32, "heads")]

    def one(agg, n, call, H, D, xdt, ydt, kind):
        ops = attn_operands(call, V, N_SRC, H, D, head_of(H), seed=900 + n)
        bias = None if kind is None else dev(random_bias(H, kind == "heads"))
        y = full((V, H * D), ydt)
        launch(call, agg, on_device(call, ops, xdt), H, y, bias)
        return y
    for first in (0, 1):
        shared = gnc.Aggregator_GAT(dptr, didx, 8, 8)
        for n, c in enumerate(calls[first:]):
            got = one(shared, n, *c)
            want = one(gnc.Aggregator_GAT(dptr, didx, c[1] * c[2], c[1] * c[2]), n, *c)
            assert torch.equal(got, want), "call %d %r on the shared handle differs from a fresh one" % (n, c)
            assert torch.isfinite(got.float()).all()


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (2, 301)])
def test_graph_capture_and_replay_of_a_biased_call(call, H, D):
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    t = on_device(call, case_operands(call, H, D), B16)
    rowwise = t["q" if call == "dot" else "xd"]
    for per_head in (True, False):
        bias = dev(random_bias(H, per_head)).clone()
        for ydt in (F32, B16):
            y = full((V, F), ydt)
            launch(call, agg, t, H, y, bias)          # warm call: the list of long rows, the scratch
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                 # (captures on a side stream: the call may neither allocate nor synchronise)
                launch(call, agg, t, H, y, bias)
            for seed in (53, 54):
                bias.copy_(dev(bf16_exact(np.random.default_rng(seed).standard_normal(tuple(bias.shape)))))
                bias[::7] = NINF
                rowwise.copy_(dev(bf16_exact(np.random.default_rng(seed + 10).standard_normal(tuple(rowwise.shape)))).to(B16))
                y.fill_(7.0)
                g.replay()
                torch.cuda.synchronize()
                eager = full((V, F), ydt)
                launch(call, agg, t, H, eager, bias)
                assert same_bits(np_of(y), np_of(eager)) and torch.isfinite(y.float()).any()


@pytest.mark.parametrize("H,D", [(8, 16), (2, 301)])
def test_an_unaligned_bias_gives_the_bits_of_an_aligned_one(H, D):
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    for call in CALLS:
        t = on_device(call, case_operands(call, H, D), F32)
        for per_head in (True, False):
            bias = dev(random_bias(H, per_head)).clone()
            bias[::5] = NINF
            assert bias.data_ptr() % 16 == 0
            buf = torch.full((bias.numel() + 3,), float("nan"), device=DEV)
            view = buf[1:1 + bias.numel()].view(bias.shape)
            view.copy_(bias)
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            keep = buf.clone()
            want = full((V, F))
            launch(call, agg, t, H, want, bias)
            by = full((V * F + 4,))
            vy = by[1:1 + V * F].view(V, F)
            launch(call, agg, t, H, vy, view)
            assert same_bits(np_of(vy), np_of(want)) and np.isfinite(np_of(want)).any()
            assert (by[:1] == 7.0).all() and (by[1 + V * F:] == 7.0).all() and same_bits(np_of(buf), np_of(keep))


def test_cabi_refusals_of_the_bias_calls_leave_y_alone():
    F = 16
    dptr, didx = dev(PTR), dev(IDX)
    gat = gnc.Aggregator_GAT(dptr, didx, F, F)
    gcn = gnc.Aggregator_GCN(dptr, didx, None, F, F)
    big = gnc.Aggregator_GAT.GATV2_MAX_FEAT + 8
    x, a, y, b = torch.zeros((N_SRC, big), device=DEV), torch.zeros(big, device=DEV), full((V, big)), torch.zeros((E, 8), device=DEV)
    L = gnc.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def dot(text, h=None, q=x, k=x, v=x, qp=big, kvp=big, xt=0, yv=y, yt=0, feat=F, heads=2, scale=0.5, bias=b, bh=2, rc_want=_lib.ERR_ARG):
        rc = L.gnnagg_dot_attn_run_bias(gat._h if h is None else h, p(q), qp, p(k), p(v), kvp, xt, p(yv), yt, feat, heads, ctypes.c_float(scale),
                                        p(bias), bh)
        err = L.gnnagg_last_error()
        assert rc == rc_want and (rc == 0 or (b"gnnagg_dot_attn_run_bias:" in err and text in err)), err

    def v2(text, h=None, xs=x, xd=x, xt=0, av=a, yv=y, yt=0, feat=F, heads=2, slope=0.2, bias=b, bh=2, rc_want=_lib.ERR_ARG):
        rc = L.gnnagg_gatv2_run_bias(gat._h if h is None else h, p(xs), p(xd), xt, p(av), p(yv), yt, feat, heads, ctypes.c_float(slope), p(bias), bh)
        err = L.gnnagg_last_error()
        assert rc == rc_want and (rc == 0 or (b"gnnagg_gatv2_run_bias:" in err and text in err)), err
    for f in (dot, v2):
        f(b"not a GAT aggregator", h=gcn._h)
        f(b"d_y", yv=None)
        f(b"x_dtype 7", xt=7)
        f(b"y_dtype -1", yt=-1)
        f(b"feat = 0", feat=0)
        f(b"feat = -4", feat=-4)
        f(b"heads = 0", heads=0)
        f(b"heads = 3", heads=3)
        f(("limit of %d" % gnc.Aggregator_GAT.GATV2_MAX_FEAT).encode(), feat=big, heads=1, bh=1)
        for n in (0, 3, 4, -1, 16):
            f(("bias_heads = %d" % n).encode(), bh=n)
        f(b"bias_heads = 2", heads=1, bh=2)
    dot(b"d_q", q=None)
    dot(b"d_k", k=None)
    dot(b"d_v", v=None)
    dot(b"q_pitch = 15", qp=15)
    dot(b"kv_pitch = -16", kvp=-16)
    for s in (float("nan"), float("inf")):
        dot(b"scale", scale=s)
    v2(b"d_xs", xs=None)
    v2(b"d_xd", xd=None)
    v2(b"d_a", av=None)
    for s in (-0.1, 1.5, float("nan")):
        v2(b"slope", slope=s)
    torch.cuda.synchronize()
    assert (y == 7.0).all()
    # a null bias ignores bias_heads and is the old entry point's call; bias_heads = 1 and = heads run
    xs = torch.randn((N_SRC, F), device=DEV)
    av = torch.randn(F, device=DEV)
    want_d, want_v = full((V, F)), full((V, F))
    gat.run_dot(xs, xs, xs, want_d, heads=2, scale=0.5)
    gat.run_v2(xs, xs, av, want_v, heads=2)
    for bh in (0, 1, 2, 99):
        yd, yv = full((V, F)), full((V, F))
        dot(b"", q=xs, k=xs, v=xs, qp=F, kvp=F, yv=yd, bias=None, bh=bh, rc_want=0)
        v2(b"", xs=xs, xd=xs, av=av, yv=yv, bias=None, bh=bh, rc_want=0)
        assert torch.equal(yd, want_d) and torch.equal(yv, want_v)
    for bh in (1, 2):
        yd, yv = full((V, F)), full((V, F))
        dot(b"", q=xs, k=xs, v=xs, qp=F, kvp=F, yv=yd, bh=bh, rc_want=0)
        v2(b"", xs=xs, xd=xs, av=av, yv=yv, bh=bh, rc_want=0)
        assert torch.equal(yd, want_d) and torch.equal(yv, want_v)       # (b is all +0.0)
    with pytest.raises(ValueError, match="bias must be"):
        gat.run_dot(xs, xs, xs, want_d, heads=2, bias=torch.zeros((E, 3), device=DEV))
    with pytest.raises(ValueError, match="operands on"):
        gat.run_v2(xs, xs, av, want_v, heads=2, bias=torch.zeros(E))


# ------------------------------------------------------------------------------------------ 8. the --edge-bias forwards
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import forward_3layer as f3  # noqa: E402


def table_bias(ptr, idx, table):
    """bias[p, h] = table[h, min(7, floor(log2(1 + degree of idx[p])))], restated in numpy"""
    deg = np.diff(ptr)[idx]
    bucket = np.minimum(7, np.floor(np.log2(1.0 + deg)).astype(np.int64))
    assert all((1 << int(bk)) <= 1 + int(d) and (bk == 7 or 1 + int(d) < (2 << int(bk))) for bk, d in zip(bucket[::97], deg[::97]))
    return np.ascontiguousarray(table.T[bucket])


@pytest.mark.parametrize("model_name", ["our_Transformer", "our_GATv2"])
@pytest.mark.parametrize("dtype,heads", [(torch.float32, 1), (torch.float32, 8), (B16, 8)])
def test_edge_bias_forward_layer_by_layer(model_name, dtype, heads):
    n_v = 2000
    ptr_t, idx_t = gnc.graph.powerlaw_csr(n_v, 30000, seed=123)
    ptr, idx = ptr_t.numpy(), idx_t.numpy()
    kw = dict(transformer=True) if model_name == "our_Transformer" else dict(gatv2=True)
    m = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN, dtype=dtype, heads=heads, edge_bias=True, **kw)
    plain = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN, dtype=dtype, heads=heads, **kw)
    assert plain.edge_bias is None and torch.equal(plain.h, m.h) and all(torch.equal(a, b) for a, b in zip(plain.weights, m.weights))
    bias = table_bias(ptr, idx, m.bias_table.cpu().numpy())
    assert m.bias_table.shape == (heads, 8) and m.edge_bias.dtype == F32 and np.array_equal(m.edge_bias.cpu().numpy(), bias)
    assert len(np.unique(np.minimum(7, np.floor(np.log2(1.0 + np.diff(ptr)[idx]))))) >= 5       # the table is in use
    m.trace = []
    y = m.forward(model_name)
    assert len(m.trace) == 3 and y.shape == (n_v, 32) and y.dtype == dtype and bool(torch.isfinite(y.float()).all())
    assert not torch.equal(y, plain.forward(model_name))
    for k, t in enumerate(m.trace):
        N = f3.DIMS[k + 1]
        assert t["bias"] is m.edge_bias
        out32 = torch.full((n_v, N), 7.0, device=DEV)
        if model_name == "our_Transformer":
            q, kk, v = t["qkv"][:, :N], t["qkv"][:, N:2 * N], t["qkv"][:, 2 * N:]
            m.at_gat.run_dot(q, kk, v, out32, heads=heads, bias=m.edge_bias)
            x = t["qkv"].float().cpu().numpy()
            ref, L, S = dot_attn_bias_ref(ptr, idx, x[:, :N], x[:, N:2 * N], x[:, 2 * N:], heads, np.float32(1.0 / math.sqrt(N // heads)), bias)
        else:
            m.at_gat.run_v2(t["feat2"], t["feat2"], t["a"], out32, heads=heads, bias=m.edge_bias)
            x = t["feat2"].float().cpu().numpy()
            ref, L, S = gatv2_bias_ref(ptr, idx, x, x, t["a"].cpu().numpy(), heads, 0.2, bias)
        assert torch.equal(t["out"], out32.to(dtype)), "layer %d: the traced output is not (one rounding of) the fp32 result" % k
        ratio = worst_ratio(out32.cpu().numpy(), ref, bias_bound(L, S, heads))
        print("%s layer %d (%s, %d heads): worst |y - ref| / bound = %.4f" % (model_name, k, dtype, heads, ratio))
        assert bool(torch.isfinite(out32).all()) and ratio <= 1.0, "layer %d: worst ratio %.3g" % (k, ratio)
    assert torch.equal(y, m.trace[-1]["out"])


def test_the_example_runs_with_edge_bias_from_the_command_line():
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (one process: the flag's way from the command line into the model; both models are judged in-process above.  --hip-graph: the
    # script itself asserts that the captured forward replays to the eager bits)
    out = subprocess.check_output([sys.executable, os.path.join(root, "examples", "forward_3layer.py"), "--model", "our_Transformer", "--edge-bias",
                                   "--heads", "8", "--iters", "1", "--hip-graph"]).decode()
    rec = json.loads(out.strip().splitlines()[-1])
    assert rec["model"] == "our_Transformer" and rec["edge_bias"] is True and rec["finite"] is True and rec["heads"] == 8
