"""GPU: the weights-out form of the two online-softmax attention calls -- gnnagg_gatv2_run_weights (Aggregator_GAT.run_v2(weights=, stats=))
and gnnagg_dot_attn_run_weights (Aggregator_GAT.run_dot(weights=, stats=)): alpha [num_e, heads] = expf(e - ms) / den per (edge position,
head) and stat [V, heads, 2] = (maximum, denominator) per (row, head) (include/gnnagg.h).  Judges, inputs and the conditions on them are
pinned on the CPU in tests/test_attn_weights_host.py.

  1. every lane geometry of geometry_census.GATV2, fp32 and bf16, on the threshold graph (rows of 0, 1, 3, 4, 5, 127, 128, 129, 512, 513,
     1025 ... edges): alpha, M and den inside their bounds, y bit-equal to the call without weights;
  2. exact cases: one edge, n copies of one source, integer operands;
  3. bias and masks for [E], [E, heads] and None: +0 weights, all-masked (row, head)s, NaN and +Inf scores, everything else bit-equal;
  4. nothing else is written: canaries, rows without edges, a graph without edges, a graph without rows;
  5. handles and streams: repeats, a long-lived handle against fresh ones, HIP-graph capture, packed q | k | v;
  6. unaligned alpha, stat and x;
  7. the refusals of the C-ABI."""
import ctypes

import numpy as np
import pytest
import torch

import geometry_census as gc
import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_attn_nonfinite_host import SCORED, SHAPES, SLOPE, attn_operands, bf16_exact, reserve_sources
from test_attn_weights_host import (BIAS_FORMS, CALLS, CENSUS, DEG, E, IDX, N_SRC, PTR, ROWS, V, bias_case_ref, case_bias, census_operands,
                                    census_ref, check_against, softmax_parts, weights_ref)
from test_gpu_attn_nonfinite import np_of, on_device, same_bits
from test_gpu_bf16_gat import DEV, dev
from test_gpu_gatv2 import full

pytestmark = pytest.mark.gpu

F32, B16 = torch.float32, torch.bfloat16
NINF = -np.inf
WORST = {}


def launch(call, agg, t, H, y, bias=None, weights=None, stats=None, slope=SLOPE):
    if call == "dot":
        return agg.run_dot(t["q"], t["k"], t["v"], y, heads=H, bias=bias, weights=weights, stats=stats)
    return agg.run_v2(t["xs"], t["xd"], t["a"], y, heads=H, slope=slope, bias=bias, weights=weights, stats=stats)


def run_w(call, agg, t, H, bias=None, ydt=F32, n_v=V, n_e=E, what=""):
    """one weights call and the same call without weights: (alpha [E, H], M [V, H], den [V, H], y) as numpy, after checking that y has the
    bits of the call without weights, that the wrapper returns the stats it was given, and that rows without edges are (-inf, +0)"""
    F = t[SCORED[call]].shape[1]
    y, y0 = full((n_v, F), ydt), full((n_v, F), ydt)
    alpha, stat = full((n_e, H)), full((n_v, H, 2))
    assert launch(call, agg, t, H, y, bias, alpha, stat) is stat
    assert launch(call, agg, t, H, y0, bias) is None
    assert same_bits(np_of(y), np_of(y0)), "%s: y differs from the call without weights" % what
    a, s = alpha.cpu().numpy(), stat.cpu().numpy()
    return a, s[:, :, 0], s[:, :, 1], np_of(y)


def assert_empty_rows(M, den, deg, what):
    e = deg == 0
    assert np.isneginf(M[e]).all() and (den[e] == 0).all() and not np.signbit(den[e]).any(), "%s: a row without edges is not (-inf, +0)" % what


# ------------------------------------------------------------------------------------------ 1. every lane geometry
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("H,D", CENSUS)
def test_every_geometry_meets_the_bound_and_keeps_y(call, H, D):
    F = H * D
    ref = census_ref(call, H, D)
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    ops = census_operands(call, H, D)
    for xdt, esize in ((F32, 4), (B16, 2)):
        what = "%s %dx%d %s %s" % (call, H, D, "fp32" if xdt == F32 else "bf16", gc.GATV2[(H, D)][esize])
        t = on_device(call, ops, xdt)
        for ydt in (F32, B16):
            alpha, M, den, _ = run_w(call, agg, t, H, ydt=ydt, what=what)
            assert_empty_rows(M, den, DEG, what)
        r = check_against((alpha, M, den), ref, PTR, what)
        WORST[call] = max(WORST.get(call, 0.0), r[0])
        # one edge: the weight and the denominator are 1.0 bit for bit
        one = np.flatnonzero(DEG == 1)
        assert (alpha[PTR[one]] == 1.0).all() and (den[one] == 1.0).all()
    print("largest fraction of the alpha bound so far, %s: %.4f" % (call, WORST[call]))


# ------------------------------------------------------------------------------------------ 2. exact cases
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("H,D", [(1, 4), (4, 16), (3, 4), (2, 50), (3, 128)])
def test_copies_of_one_source_and_integer_scores_are_exact(call, H, D):
    """n copies of one source: every weight 1 / n, den = n, M the one score; small-integer operands with power-of-two scale and slope 0.5
    (every product, sum and score exact in fp32): M is the float64 maximum bit for bit, on every row length"""
    F = H * D
    rng = np.random.default_rng(H * D)
    # rows of 4, 128 and 1024 copies, an empty row, then the threshold graph's rows
    lens = [4, 128, 0, 1024]
    ptr = np.concatenate([[0], np.cumsum(lens), np.cumsum(lens)[-1] + PTR[1:]]).astype(np.int32)
    idx = np.concatenate([np.repeat([7, 3, 11], [4, 128, 1024]), IDX]).astype(np.int32)
    n_v, n_e = len(ptr) - 1, len(idx)
    deg = np.diff(ptr)
    ints = lambda shape: rng.integers(-2, 3, shape).astype(np.float32)
    if call == "dot":
        scale = np.float32(0.25)
        ops = dict(q=ints((n_v, F)), k=ints((N_SRC, F)), v=ints((N_SRC, F)))
        rows = np.repeat(np.arange(n_v), deg)
        e = float(scale) * (ops["q"].astype(np.float64)[rows] * ops["k"].astype(np.float64)[idx]).reshape(n_e, H, D).sum(axis=2)
    else:
        ops = dict(xs=ints((N_SRC, F)), xd=ints((n_v, F)), a=ints((H, D)))
        rows = np.repeat(np.arange(n_v), deg)
        z = ops["xd"].astype(np.float64)[rows] + ops["xs"].astype(np.float64)[idx]
        e = (ops["a"].astype(np.float64).reshape(1, F) * np.where(z > 0.5 * z, z, 0.5 * z)).reshape(n_e, H, D).sum(axis=2)
    assert np.array_equal(e.astype(np.float32).astype(np.float64), e)      # the scores are fp32 numbers
    a_ref, M_ref, d_ref = softmax_parts(ptr, e)
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    for xdt in (F32, B16):
        t = on_device(call, ops, xdt)
        y, y0, alpha, stat = full((n_v, F)), full((n_v, F)), full((n_e, H)), full((n_v, H, 2))
        if call == "dot":
            agg.run_dot(t["q"], t["k"], t["v"], y, heads=H, scale=float(scale), weights=alpha, stats=stat)
            agg.run_dot(t["q"], t["k"], t["v"], y0, heads=H, scale=float(scale))
        else:
            agg.run_v2(t["xs"], t["xd"], t["a"], y, heads=H, slope=0.5, weights=alpha, stats=stat)
            agg.run_v2(t["xs"], t["xd"], t["a"], y0, heads=H, slope=0.5)
        assert torch.equal(y, y0)
        al, st = alpha.cpu().numpy(), stat.cpu().numpy()
        has = deg > 0
        assert np.array_equal(st[has, :, 0].astype(np.float64), M_ref[has]), "M is not the float64 maximum bit for bit"
        assert_empty_rows(st[:, :, 0], st[:, :, 1], deg, "integer %s %dx%d" % (call, H, D))
        for r, n in ((0, 4), (1, 128), (3, 1024)):
            assert (al[ptr[r]:ptr[r + 1]] == np.float32(1.0) / np.float32(n)).all() and (st[r, :, 1] == n).all()
            assert np.array_equal(st[r, :, 0].astype(np.float64), e[ptr[r]])
        # every other weight: exact scores leave the exp (a few ulp), the division (half an ulp) and the denominator's sum, whose worst case
        # over n <= 1573 fp32 additions is n * 2^-24 < 1e-4 relative.  (Integer scores spread by more than 60: weights that fp32 holds as
        # subnormals or zeros are left out.)
        ok = a_ref > 1e-20
        assert np.allclose(al[ok], a_ref[ok], rtol=1e-4, atol=0)


# ------------------------------------------------------------------------------------------ 3. bias and masks
def masked_bias(form, H, kind, shift=0):
    """(bias of one form with non-finite entries, the (row, head)s they reach [V, H] bool, the rows masked whole [V, H] bool): -inf on
    every fifth edge and on ALL edges of every seventh row with edges (head 0 only where the bias has heads); kind "inf" / "nan": that value
    on one edge of every third row with edges instead of the whole-row mask"""
    b = np.zeros(E, np.float32) if form == "none" else np.array(case_bias(form, H), np.float32, copy=True)
    b2 = b.reshape(E, -1)
    cols = b2.shape[1]
    hit = np.zeros((V, cols), bool)
    whole = np.zeros((V, cols), bool)
    b2[shift::5] = NINF
    rows_with = np.flatnonzero(DEG > 1)
    if kind == "mask":
        for r in rows_with[::7]:
            b2[PTR[r]:PTR[r + 1], 0] = NINF
            whole[r, 0] = True
    else:
        for r in rows_with[1::3]:
            b2[PTR[r] + (r % DEG[r]), cols - 1] = np.inf if kind == "inf" else np.nan
            hit[r, cols - 1] = True
    # a row of one edge at a multiple of five is masked whole too
    e_mask = np.isneginf(b2)
    starts = PTR[:-1][DEG > 0]
    whole[DEG > 0] |= np.logical_and.reduceat(e_mask, starts, axis=0)
    bc = lambda m: np.broadcast_to(m, (V, H)) if cols == 1 else m
    return b, bc(hit), bc(whole)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("H,D", [(1, 8), (8, 16), (4, 128), (4, 3), (2, 301)])
@pytest.mark.parametrize("form", BIAS_FORMS[1:])
def test_bias_masks_and_non_finite_scores(call, H, D, form):
    assert (H, D) in SHAPES
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    ops = census_operands(call, H, D)
    clean_bias = case_bias(form, H)
    ref = bias_case_ref(call, H, D, form)
    for xdt in (F32, B16):
        t = on_device(call, ops, xdt)
        what = "%s %dx%d bias per %s, %s" % (call, H, D, form, xdt)
        a0, M0, d0, y0 = run_w(call, agg, t, H, dev(clean_bias), what=what)
        check_against((a0, M0, d0), ref, PTR, what)
        for kind in ("mask", "inf", "nan"):
            b, hit, whole = masked_bias(form, H, kind)
            a1, M1, d1, y1 = run_w(call, agg, t, H, dev(b), what=what + " " + kind)
            mref = weights_ref(call, PTR, IDX, ops, H, b)
            masked = np.broadcast_to(np.isneginf(b.reshape(E, -1)), (E, H))
            bad = (hit | whole)[ROWS]
            # a masked edge is +0, the bit pattern, unless its (row, head) is NaN as a whole
            assert (a1[masked & ~bad] == 0).all() and not np.signbit(a1[masked & ~bad]).any()
            assert np.isnan(a1[bad]).all() and not np.isnan(a1[~bad]).any(), what
            assert np.array_equal(np.isnan(mref[1]), bad)
            # all masked: (-inf, +0); a +Inf or NaN score: a NaN denominator
            assert np.isneginf(M1[whole & ~hit]).all() and (d1[whole & ~hit] == 0).all() and not np.signbit(d1[whole & ~hit]).any()
            assert np.isnan(d1[hit]).all()
            # the other weights: inside the bound of the judge with -inf scores, which is the judge of the graph without those edges
            fin = ~bad
            got = (np.where(fin, a1, 0), np.where(hit | whole, 0, M1), np.where(hit | whole, 0, d1))
            want = (mref[0], np.where(fin, mref[1], 0), np.where(hit | whole, 0, mref[2]), np.where(hit | whole, 0, mref[3]), mref[4])
            check_against(got, want, PTR, what + " " + kind)
        # (row, head)s that no non-finite value reaches: the bits of the clean run.  Only the inf / nan edge is non-finite here.
        for kind, val in (("inf", np.inf), ("nan", np.nan)):
            b = np.array(clean_bias, np.float32, copy=True)
            b2 = b.reshape(E, -1)
            rows_hit = np.flatnonzero(DEG > 1)[1::3]
            for r in rows_hit:
                b2[PTR[r] + (r % DEG[r]), -1] = val
            a1, M1, d1, y1 = run_w(call, agg, t, H, dev(b), what=what + " lone " + kind)
            reach = np.zeros((V, H), bool)
            reach[rows_hit, slice(None) if b2.shape[1] == 1 else H - 1] = True
            assert np.isnan(a1[reach[ROWS]]).all() and same_bits(a1[~reach[ROWS]], a0[~reach[ROWS]])
            assert same_bits(M1[~reach], M0[~reach]) and same_bits(d1[~reach], d0[~reach])
            cols = np.repeat(reach, D, axis=1)
            assert np.isnan(y1[cols]).all() and same_bits(y1[~cols], y0[~cols])


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("H,D", [(8, 16), (2, 301)])
def test_no_bias_with_non_finite_operands(call, H, D):
    """bias None (the null-bias branch of the weights arm): -Inf, +Inf and NaN scores made by the scored operand of reserved sources"""
    F, h = H * D, H // 2
    idx, reserved = reserve_sources(IDX, N_SRC)
    rows_hit = np.flatnonzero(DEG > 1)[::4]
    idx = idx.copy()
    pos = np.array([PTR[r] + (r % DEG[r]) for r in rows_hit])
    idx[pos] = reserved[0]
    agg = gnc.Aggregator_GAT(dev(PTR), dev(idx), F, F)
    clean = attn_operands(call, V, N_SRC, H, D, h, seed=H * D + 1)
    t0 = on_device(call, clean, F32)
    a0, M0, d0, y0 = run_w(call, agg, t0, H, what="clean")
    check_against((a0, M0, d0), weights_ref(call, PTR, idx, clean, H), PTR, "%s %dx%d, no bias, reserved sources" % (call, H, D))
    reach = np.zeros((V, H), bool)
    reach[rows_hit, h] = True
    for val in (NINF, np.inf, np.nan):
        ops = dict(clean)
        ops[SCORED[call]] = clean[SCORED[call]].copy()
        ops[SCORED[call]][reserved[0], h * D] = val
        a1, M1, d1, _ = run_w(call, agg, on_device(call, ops, F32), H, what="%r" % val)
        other = ~reach[ROWS]
        assert same_bits(a1[other], a0[other]) and same_bits(M1[~reach], M0[~reach]) and same_bits(d1[~reach], d0[~reach])
        if val == NINF:
            assert (a1[pos, h] == 0).all() and not np.signbit(a1[pos, h]).any() and np.isfinite(a1).all()
            ref = weights_ref(call, PTR, idx, ops, H)
            check_against((a1, M1, d1), ref, PTR, "%s %dx%d, -Inf operand" % (call, H, D))
        else:
            assert np.isnan(a1[reach[ROWS]]).all() and np.isnan(d1[reach]).all()


# ------------------------------------------------------------------------------------------ 4. nothing else is written
@pytest.mark.parametrize("call", CALLS)
def test_canaries_and_graphs_without_edges_or_rows(call):
    H, D = 3, 50
    F = H * D
    ops = census_operands(call, H, D)
    t = on_device(call, ops, F32)
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    pad = 64
    abuf, sbuf = full((E * H + 2 * pad,)), full((V * H * 2 + 2 * pad,))
    alpha, stat = abuf[pad:pad + E * H].view(E, H), sbuf[pad:pad + V * H * 2].view(V, H, 2)
    y = full((V, F))
    launch(call, agg, t, H, y, None, alpha, stat)
    for buf, n in ((abuf, E * H), (sbuf, V * H * 2)):
        assert (buf[:pad] == 7.0).all() and (buf[pad + n:] == 7.0).all()
    want = run_w(call, agg, t, H)
    assert same_bits(alpha.cpu().numpy(), want[0]) and same_bits(stat.cpu().numpy()[:, :, 0], want[1])
    assert_empty_rows(want[1], want[2], DEG, call)
    assert not (stat == 7.0).any()          # every (row, head) pair is written
    # a graph without edges: every pair is (-inf, +0), y is +0, alpha has no element
    n_v = 9
    agg0 = gnc.Aggregator_GAT(dev(np.zeros(n_v + 1, np.int32)), dev(np.zeros(0, np.int32)), F, F)
    y, w, s = full((n_v, F)), torch.zeros((0, H), device=DEV), full((n_v, H, 2))
    launch(call, agg0, t, H, y, None, w, s)
    s = s.cpu().numpy()
    assert_empty_rows(s[:, :, 0], s[:, :, 1], np.zeros(n_v, np.int64), "no edges")
    assert (y == 0).all()
    # a graph without rows, through the C-ABI (tensors without elements have no pointer): OK, nothing written
    aggv = gnc.Aggregator_GAT(dev(np.zeros(1, np.int32)), dev(np.zeros(0, np.int32)), F, F)
    L = gnc.lib()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    can = full((8,))
    x = t[SCORED[call]]
    if call == "dot":
        rc = L.gnnagg_dot_attn_run_weights(aggv._h, p(x), F, p(x), p(x), F, 0, p(can), 0, F, H, ctypes.c_float(0.5), None, 1, p(can), p(can))
    else:
        rc = L.gnnagg_gatv2_run_weights(aggv._h, p(x), p(x), 0, p(t["a"]), p(can), 0, F, H, ctypes.c_float(0.2), None, 1, p(can), p(can))
    torch.cuda.synchronize()
    assert rc == 0 and (can == 7.0).all()


# ------------------------------------------------------------------------------------------ 5. handles and streams
def test_a_long_lived_handle_against_fresh_ones_and_three_calls_in_a_row():
    dptr, didx = dev(PTR), dev(IDX)
    # (call, H, D, x dtype, y dtype, bias form, weights?)
    calls = [("dot", 4, 8, B16, F32, "head", True), ("v2", 1, 8, F32, F32, "none", False), ("dot", 1, 602, F32, B16, "edge", True),
             ("v2", 8, 16, B16, B16, "head", True), ("dot", 8, 16, F32, F32, "none", True), ("v2", 2, 301, F32, F32, "edge", False),
             ("v2", 2, 301, F32, F32, "edge", True), ("dot", 8, 32, F32, F32, "head", False), ("v2", 8, 16, B16, B16, "none", True),
             ("dot", 4, 8, B16, F32, "none", False), ("v2", 1, 8, F32, F32, "head", True), ("dot", 1, 1024, B16, B16, "none", True)]

    def one(agg, n, call, H, D, xdt, ydt, form, want_w):
        ops = attn_operands(call, V, N_SRC, H, D, H // 2, seed=300 + n)
        bias = None if form == "none" else dev(case_bias(form, H))
        y, w, s = full((V, H * D), ydt), full((E, H)), full((V, H, 2))
        launch(call, agg, on_device(call, ops, xdt), H, y, bias, w if want_w else None, s if want_w else None)
        return y, w, s
    for first in (0, 1):
        shared = gnc.Aggregator_GAT(dptr, didx, 8, 8)
        for n, c in enumerate(calls[first:]):
            got = one(shared, n, *c)
            for k in range(2):       # three calls in a row: the same bits
                again = one(shared, n, *c)
                assert all(same_bits(np_of(a), np_of(b)) for a, b in zip(got, again)), "call %d %r differs on its repeat %d" % (n, c, k)
            F = c[1] * c[2]
            want = one(gnc.Aggregator_GAT(dptr, didx, F, F), n, *c)
            assert all(same_bits(np_of(a), np_of(b)) for a, b in zip(got, want)), "call %d %r on the shared handle differs from a fresh one" % (n, c)
            assert torch.isfinite(got[0].float()).all() and (not c[6] or torch.isfinite(got[1]).all())


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (2, 301)])
def test_graph_capture_and_replay_of_a_weights_call(call, H, D):
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    t = on_device(call, census_operands(call, H, D), B16)
    rowwise = t["q" if call == "dot" else "xd"]
    for form in BIAS_FORMS:
        bias = None if form == "none" else dev(case_bias(form, H)).clone()
        y, w, s = full((V, F)), full((E, H)), full((V, H, 2))
        launch(call, agg, t, H, y, bias, w, s)          # warm call: the list of long rows, the scratch
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                       # (captures on a side stream: the call may neither allocate nor synchronise)
            launch(call, agg, t, H, y, bias, w, s)
        for seed in (53, 54):
            rowwise.copy_(dev(bf16_exact(np.random.default_rng(seed + 10).standard_normal(tuple(rowwise.shape)))).to(B16))
            y.fill_(7.0)
            w.zero_()
            s.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            ey, ew, es = full((V, F)), full((E, H)), full((V, H, 2))
            launch(call, agg, t, H, ey, bias, ew, es)
            assert same_bits(np_of(y), np_of(ey)) and same_bits(np_of(w), np_of(ew)) and same_bits(np_of(s), np_of(es))
            assert torch.isfinite(w).all() and (w > 0).any()


@pytest.mark.parametrize("dt", [F32, B16])
def test_row_views_of_one_packed_tensor_serve_run_dot(dt):
    H, D = 8, 16
    F = H * D
    ops = census_operands("dot", H, D)
    n = max(V, N_SRC)
    packed = torch.zeros((n, 3 * F), device=DEV, dtype=dt)
    packed[:V, :F] = dev(ops["q"]).to(dt)
    packed[:N_SRC, F:2 * F] = dev(ops["k"]).to(dt)
    packed[:N_SRC, 2 * F:] = dev(ops["v"]).to(dt)
    views = dict(q=packed[:, :F], k=packed[:, F:2 * F], v=packed[:, 2 * F:])
    assert not views["k"].is_contiguous()
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    got = run_w("dot", agg, views, H, what="packed")
    want = run_w("dot", agg, on_device("dot", ops, dt), H, what="apart")
    assert all(same_bits(a, b) for a, b in zip(got, want))
    check_against(got[:3], census_ref("dot", H, D), PTR, "packed q | k | v, %s" % dt)


# ------------------------------------------------------------------------------------------ 6. unaligned operands
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("H,D", [(8, 16), (3, 50), (3, 4)])
def test_unaligned_alpha_stat_and_x_give_the_aligned_bits(call, H, D):
    F = H * D
    agg = gnc.Aggregator_GAT(dev(PTR), dev(IDX), F, F)
    ops = census_operands(call, H, D)
    for dt in (F32, B16):
        t = on_device(call, ops, dt)
        assert all(x.data_ptr() % 16 == 0 for x in t.values())
        want = run_w(call, agg, t, H, dev(case_bias("head", H)))
        # every operand at an odd element offset: x_aligned = 0, alpha and stat 4 bytes off a 16-byte boundary
        tu = {}
        for k, x in t.items():
            buf = torch.zeros(x.numel() + 3, device=DEV, dtype=x.dtype)
            tu[k] = buf[1:1 + x.numel()].view(x.shape)
            tu[k].copy_(x)
        abuf, sbuf = full((E * H + 4,)), full((V * H * 2 + 4,))
        alpha, stat = abuf[1:1 + E * H].view(E, H), sbuf[3:3 + V * H * 2].view(V, H, 2)
        assert alpha.data_ptr() % 16 == 4 and stat.data_ptr() % 16 == 12 and tu[SCORED[call]].data_ptr() % 16 != 0
        y = full((V, F))
        launch(call, agg, tu, H, y, dev(case_bias("head", H)), alpha, stat)
        s = stat.cpu().numpy()
        assert same_bits(alpha.cpu().numpy(), want[0]) and same_bits(s[:, :, 0], want[1]) and same_bits(s[:, :, 1], want[2])
        assert same_bits(np_of(y), want[3])
        assert (abuf[:1] == 7.0).all() and (abuf[1 + E * H:] == 7.0).all() and (sbuf[:3] == 7.0).all() and (sbuf[3 + V * H * 2:] == 7.0).all()


# ------------------------------------------------------------------------------------------ 7. refusals through the C-ABI
def test_cabi_refusals_of_the_weights_calls_leave_the_outputs_alone():
    F, H = 16, 2
    dptr, didx = dev(PTR), dev(IDX)
    gat = gnc.Aggregator_GAT(dptr, didx, F, F)
    gcn = gnc.Aggregator_GCN(dptr, didx, None, F, F)
    big = gnc.Aggregator_GAT.GATV2_MAX_FEAT + 8
    x, a, y, b = torch.zeros((N_SRC, big), device=DEV), torch.zeros(big, device=DEV), full((V, big)), torch.zeros((E, 8), device=DEV)
    w, s = full((E, 8)), full((V, 8, 2))
    L = gnc.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def dot(text, h=None, q=x, yv=y, xt=0, feat=F, heads=H, scale=0.5, bias=b, bh=H, wv=w, sv=s, qp=big):
        rc = L.gnnagg_dot_attn_run_weights(gat._h if h is None else h, p(q), qp, p(x), p(x), big, xt, p(yv), 0, feat, heads, ctypes.c_float(scale),
                                           p(bias), bh, p(wv), p(sv))
        err = L.gnnagg_last_error()
        assert rc == _lib.ERR_ARG and b"gnnagg_dot_attn_run_weights:" in err and text in err, err

    def v2(text, h=None, q=x, yv=y, xt=0, feat=F, heads=H, slope=0.2, bias=b, bh=H, wv=w, sv=s):
        rc = L.gnnagg_gatv2_run_weights(gat._h if h is None else h, p(q), p(x), xt, p(a), p(yv), 0, feat, heads, ctypes.c_float(slope), p(bias), bh,
                                        p(wv), p(sv))
        err = L.gnnagg_last_error()
        assert rc == _lib.ERR_ARG and b"gnnagg_gatv2_run_weights:" in err and text in err, err
    for f in (dot, v2):
        f(b"d_alpha", wv=None)
        f(b"d_stat", sv=None)
        f(b"d_alpha", wv=None, sv=None)
        f(b"d_alpha", wv=None, bias=None)
        for n in (0, 3, -1, 16):
            f(("bias_heads = %d" % n).encode(), bh=n)
        f(b"bias_heads = 2", heads=1, bh=2)
        f(b"not a GAT aggregator", h=gcn._h)
        f(b"d_y", yv=None)
        f(b"x_dtype 7", xt=7)
        f(b"heads = 3", heads=3)
        f(("limit of %d" % gnc.Aggregator_GAT.GATV2_MAX_FEAT).encode(), feat=big, heads=1, bh=1)
    dot(b"d_q", q=None)
    dot(b"q_pitch = 15", qp=15)
    dot(b"scale", scale=float("nan"))
    v2(b"d_xs", q=None)
    v2(b"slope", slope=1.5)
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (w == 7.0).all() and (s == 7.0).all()
    # the same arguments with everything in place run: the refusals above were the arguments', not the setting's
    rc = L.gnnagg_dot_attn_run_weights(gat._h, p(x), big, p(x), p(x), big, 0, p(y), 0, F, H, ctypes.c_float(0.5), None, 3, p(w), p(s))
    assert rc == 0, L.gnnagg_last_error()           # (d_bias == NULL: bias_heads is ignored)
    torch.cuda.synchronize()
    assert (w.view(-1)[:E * H] != 7.0).all() and (w.view(-1)[E * H:] == 7.0).all()
    m, d = s.view(-1)[:V * H * 2].view(V, H, 2)[:, :, 0].cpu().numpy(), s.view(-1)[:V * H * 2].view(V, H, 2)[:, :, 1].cpu().numpy()
    assert ((m == 0) | np.isneginf(m)).all() and np.array_equal(d, np.repeat(DEG[:, None], H, axis=1)) and (s.view(-1)[V * H * 2:] == 7.0).all()
