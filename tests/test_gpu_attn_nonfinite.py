"""GPU: non-finite scores and features on the two online-softmax attention calls -- gnnagg_gatv2_run (Aggregator_GAT.run_v2,
csrc/agg_gatv2.hip) and gnnagg_dot_attn_run (Aggregator_GAT.run_dot, csrc/agg_dot.hip) -- against the contract of include/gnnagg.h
("non-finite" in both paragraphs): the result has the class map (finite / +Inf / -Inf / NaN, element for element) of the two-pass float64
formulas.  Generators, judges and the conditions on the inputs are pinned on the CPU in tests/test_attn_nonfinite_host.py.

Every case runs both calls with fp32 and bf16 inputs into an fp32 and a bf16 y pre-filled with 7.0, and the WHOLE output is judged:
  a. edges masked by position (a -Inf score in one head): the judge's class map; finite elements within 1e-5 (1 + L) S of the reference on
     the graph with the masked edges deleted; the other heads bit-equal to the clean run; fully masked (row, head)s NaN;
  b. one +Inf / NaN score, or one +Inf / NaN q / xd element: exactly the (row, head)s that reach it are NaN, the rest bit-equal;
  c. +Inf columns in every source row of v, and of k / xs;
  d. rows that must not be read: source 0 (the id of padded lanes), a source behind the last id, the q / xd rows of rows without edges;
  e. the element-wise load path (unaligned, pitched views): the bits of the aligned run.
Found by group a on the kernels as they were: a batch (a lane group's chunk, a segment) whose scores are all -Inf while the running maximum
is still -Inf formed expf(-Inf - -Inf) = NaN and poisoned the row."""
import functools
import time

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from test_attn_nonfinite_host import (N_RESERVED, PATTERNS, ROWWISE, SCORED, SEG, SHAPES, SLOPE, assert_spread, attn_operands, full_ref,
                                      geometry, mask_edges, masked_case, masked_judge, pattern_id, reserve_sources)
from test_dot_attn_host import dot_attn_bound
from test_gatv2_host import gatv2_bound, worst_ratio
from test_gpu_bf16_gat import DEV, dev
from test_gpu_dot_attn import pitched
from test_gpu_gatv2 import full, threshold_graph
from test_nonfinite_host import assert_same_classes, inf_columns

pytestmark = pytest.mark.gpu

F32, B16 = torch.float32, torch.bfloat16
CALLS = ("dot", "v2")
PTR, IDX, N_SRC = threshold_graph(n_src_extra=300)
V = len(PTR) - 1
DEG = np.diff(PTR)
EMPTY = DEG == 0
LONGEST = int(np.argmax(DEG))


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print("\ntests/test_gpu_attn_nonfinite.py wall time: %.1f s" % (time.time() - t0))


def test_the_graph_has_the_rows_the_cases_need():
    for n in (0, 1, 3, 4, 5, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1, 3 * SEG + 37):
        assert (DEG == n).any()
    for t in gnc.Aggregator_GAT.GATV2_THRESHOLDS:
        assert (DEG == t - 1).any() and (DEG == t).any() and (DEG == t + 1).any()
    assert DEG[LONGEST] == 3 * SEG + 37 and 6000 < len(IDX) < 9000 and IDX.max() == N_SRC - 1 and N_SRC - N_RESERVED - 1 >= V


def head_of(H):
    return H // 2   # the head that is masked or poisoned: a middle one where there are several


def np_of(y):
    return y.float().cpu().numpy()


def same_bits(a, b):
    """equal values, NaN = NaN, and the same sign on zeros"""
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b))


def on_device(call, ops, dt):
    return {k: dev(v) if k == "a" else dev(v).to(dt) for k, v in ops.items()}


def launch(call, agg, t, H, y):
    if call == "dot":
        agg.run_dot(t["q"], t["k"], t["v"], y, heads=H)
    else:
        agg.run_v2(t["xs"], t["xd"], t["a"], y, heads=H, slope=SLOPE)


def run_both_y(call, agg, ops, H, dt, what):
    """the fp32 y of one run as numpy, after checking that the bf16 y of the same run is one rounding of it (NaN = NaN) and that rows
    without edges are +0; ops hold bf16-exact values, so dt = bf16 runs the same numbers"""
    F = ops[SCORED[call]].shape[1]
    t = on_device(call, ops, dt)
    y32, y16 = full((V, F)), full((V, F), B16)
    launch(call, agg, t, H, y32)
    launch(call, agg, t, H, y16)
    assert same_bits(np_of(y16), np_of(y32.to(B16))), "%s: the bf16 y is not one rounding of the fp32 y" % what
    y = y32.cpu().numpy()
    assert np.all(y[EMPTY] == 0) and not np.signbit(y[EMPTY]).any(), "%s: a row without edges is not +0" % what
    return y


@functools.lru_cache(maxsize=None)
def spread_of_the_unmasked_graph(call, H, D, seed):
    """The condition on the inputs (finite scores of a (row, head) within 60 of each other), asserted once per shape and call on the graph
    with nothing masked: a masked case keeps the sources of its unmasked edges, so its finite scores are a subset of these."""
    idx, _ = reserve_sources(IDX, N_SRC)
    return assert_spread(call, PTR, idx, attn_operands(call, V, N_SRC, H, D, head_of(H), seed), H, "%s %dx%d" % (call, H, D))


def tags(call, H, D, dt, extra=""):
    return "%s %dx%d %s x%s" % (call, H, D, "bf16" if dt == B16 else "fp32", extra and ", " + extra)


# ------------------------------------------------------------------------------------------ 0. the clean run on this graph is judged once
@pytest.mark.parametrize("H,D", SHAPES)
def test_the_clean_run_is_within_the_bound(H, D):
    F, h = H * D, head_of(H)
    idx, _ = reserve_sources(IDX, N_SRC)
    agg = gnc.Aggregator_GAT(dev(PTR), dev(idx), F, F)
    for call in CALLS:
        ops = attn_operands(call, V, N_SRC, H, D, h, seed=F)
        assert_spread(call, PTR, idx, ops, H, "%s %dx%d" % (call, H, D))
        ref, L, S = full_ref(call, PTR, idx, ops, H)
        bound = (dot_attn_bound if call == "dot" else gatv2_bound)(L, S, H)
        for dt in (F32, B16):
            y = run_both_y(call, agg, ops, H, dt, tags(call, H, D, dt))
            ratio = worst_ratio(y, ref, bound)
            print("%s: worst |y - ref| / bound = %.4f" % (tags(call, H, D, dt), ratio))
            assert np.isfinite(y).all() and ratio <= 1.0


# ------------------------------------------------------------------------------------------ a. masked edges by position
@pytest.mark.parametrize("pattern", PATTERNS, ids=pattern_id)
@pytest.mark.parametrize("H,D", SHAPES)
def test_masked_edges_are_weights_of_zero_wherever_they_stand(H, D, pattern):
    F, h = H * D, head_of(H)
    sl = slice(h * D, (h + 1) * D)
    other = np.r_[0:h * D, (h + 1) * D:F]
    mask = mask_edges(PTR, pattern)
    agg = None
    for call in CALLS:
        idx, clean, masked = masked_case(call, PTR, IDX, N_SRC, H, D, h, mask, seed=F)
        if agg is None:
            agg = gnc.Aggregator_GAT(dev(PTR), dev(idx), F, F)      # (idx is the same for both calls)
        spread_of_the_unmasked_graph(call, H, D, F)
        ref_full, ref_del, bound, gone = masked_judge(call, PTR, idx, mask, masked, H, h)
        fin = np.isfinite(ref_full)
        for dt in (F32, B16):
            what = tags(call, H, D, dt, pattern_id(pattern))
            y_clean = run_both_y(call, agg, clean, H, dt, what + " (clean)")
            y = run_both_y(call, agg, masked, H, dt, what)
            assert np.isfinite(y_clean).all()
            assert_same_classes(y[:, sl], ref_full, what)
            ratio = worst_ratio(y[:, sl][fin], ref_del[fin], bound[fin])
            print("%s: worst |y - ref| / bound on the masked head = %.4f" % (what, ratio))
            assert ratio <= 1.0, "%s: worst ratio %.3g against the bound of the graph with the masked edges deleted" % (what, ratio)
            assert np.isnan(y[gone][:, sl]).all(), "%s: a fully masked (row, head) is not NaN" % what
            assert same_bits(y[:, other], y_clean[:, other]), "%s: another head differs from the clean run" % what


# ------------------------------------------------------------------------------------------ b. +Inf and NaN scores
def poisoned_rows():
    """every third row with edges, and the longest"""
    rows = np.flatnonzero(DEG > 0)[::3]
    return np.union1d(rows, [LONGEST])


@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("H,D", SHAPES)
def test_an_inf_or_nan_score_makes_exactly_its_row_heads_nan(H, D, bad):
    F, h = H * D, head_of(H)
    sl = slice(h * D, (h + 1) * D)
    rows = poisoned_rows()
    base, reserved = reserve_sources(IDX, N_SRC)
    special = int(reserved[0])
    expect_nan = np.zeros((V, F), bool)
    expect_nan[rows, sl] = True
    for where in ("first", "middle", "last"):
        pos = {"first": PTR[:-1], "middle": PTR[:-1] + DEG // 2, "last": PTR[1:] - 1}[where][rows]
        idx = base.copy()
        idx[pos] = special
        assert idx[PTR[LONGEST + 1] - 1] == special or where != "last"
        agg = gnc.Aggregator_GAT(dev(PTR), dev(idx), F, F)
        for call in CALLS:
            clean = attn_operands(call, V, N_SRC, H, D, h, seed=F + 1)
            poisoned = dict(clean)
            poisoned[SCORED[call]] = clean[SCORED[call]].copy()
            poisoned[SCORED[call]][special, h * D] = bad      # q[:, hD] > 0 / a[h, 0] > 0: a +Inf element is a +Inf score
            for dt in (F32, B16):
                what = tags(call, H, D, dt, "%r on the %s edge" % (bad, where))
                y_clean = run_both_y(call, agg, clean, H, dt, what + " (clean)")
                y = run_both_y(call, agg, poisoned, H, dt, what)
                assert np.isfinite(y_clean).all()
                assert np.array_equal(np.isnan(y), expect_nan), "%s: NaN in other places than the (row, head)s that reach the source" % what
                assert same_bits(y[~expect_nan], y_clean[~expect_nan]), "%s: an element the source does not reach differs from the clean run" % what
    # one q / xd row: that row only
    qrows = np.array([LONGEST, int(np.flatnonzero(DEG == 1)[0]), int(np.flatnonzero(DEG == 5)[0]), int(np.flatnonzero(DEG == 2 * SEG)[0])])
    expect_nan = np.zeros((V, F), bool)
    expect_nan[qrows, sl] = True
    agg = gnc.Aggregator_GAT(dev(PTR), dev(base), F, F)
    for call in CALLS:
        clean = attn_operands(call, V, N_SRC, H, D, h, seed=F + 1)
        poisoned = dict(clean)
        poisoned[ROWWISE[call]] = clean[ROWWISE[call]].copy()
        poisoned[ROWWISE[call]][qrows, h * D] = bad
        for dt in (F32, B16):
            what = tags(call, H, D, dt, "%r in %s" % (bad, ROWWISE[call]))
            y_clean = run_both_y(call, agg, clean, H, dt, what + " (clean)")
            y = run_both_y(call, agg, poisoned, H, dt, what)
            assert np.array_equal(np.isnan(y), expect_nan), "%s: NaN in other places than the poisoned rows' head" % what
            assert same_bits(y[~expect_nan], y_clean[~expect_nan]), "%s: another (row, head) differs from the clean run" % what


# ------------------------------------------------------------------------------------------ c. Inf columns
@pytest.mark.parametrize("H,D", SHAPES)
def test_inf_columns_in_every_source_row(H, D):
    F, h = H * D, head_of(H)
    idx, _ = reserve_sources(IDX, N_SRC)
    agg = gnc.Aggregator_GAT(dev(PTR), dev(idx), F, F)
    every_head, edge_heads = inf_columns(F, H), sorted({0, F - 1})
    for call in CALLS:
        clean = attn_operands(call, V, N_SRC, H, D, h, seed=F + 2)
        y_clean = {dt: run_both_y(call, agg, clean, H, dt, tags(call, H, D, dt, "clean")) for dt in (F32, B16)}
        if call == "dot":    # in v: +Inf on every row with edges, never NaN (every weight is positive), the other columns untouched
            ops = dict(clean, v=clean["v"].copy())
            ops["v"][:, every_head] = np.inf
            keep = np.setdiff1d(np.arange(F), every_head)
            for dt in (F32, B16):
                what = tags(call, H, D, dt, "+Inf columns in v")
                y = run_both_y(call, agg, ops, H, dt, what)
                assert not np.isnan(y).any(), "%s: NaN" % what
                assert np.isposinf(y[~EMPTY][:, every_head]).all(), "%s: an Inf column of a row with edges is not +Inf" % what
                assert same_bits(y[:, keep], y_clean[dt][:, keep]), "%s: another column differs from the clean run" % what
        for cols in (every_head, edge_heads):   # in k / xs: the class map of the judge; heads without such a column untouched
            ops = dict(clean)
            ops[SCORED[call]] = clean[SCORED[call]].copy()
            ops[SCORED[call]][:, cols] = np.inf
            ref = full_ref(call, PTR, idx, ops, H)[0]
            hit = np.zeros(F, bool)
            for c in cols:
                hit[c // D * D:(c // D + 1) * D] = True
            assert np.isnan(ref[~EMPTY][:, hit]).all() and np.isfinite(ref[:, ~hit]).all()   # (all +Inf, all -Inf or mixed: NaN either way)
            for dt in (F32, B16):
                what = tags(call, H, D, dt, "+Inf columns %s in %s" % (cols, SCORED[call]))
                y = run_both_y(call, agg, ops, H, dt, what)
                assert_same_classes(y, ref, what)
                assert same_bits(y[:, ~hit], y_clean[dt][:, ~hit]), "%s: a head without an Inf column differs from the clean run" % what


# ------------------------------------------------------------------------------------------ d. what must not be read
@pytest.mark.parametrize("H,D", SHAPES)
def test_rows_that_no_edge_names_are_never_read_into_a_result(H, D):
    F, h = H * D, head_of(H)
    idx, _ = reserve_sources(IDX, N_SRC)
    idx[idx == 0] = 1              # padded lanes carry id 0: no edge names it here
    assert (idx != 0).all() and idx.max() < N_SRC
    agg = gnc.Aggregator_GAT(dev(PTR), dev(idx), F, F)
    for call in CALLS:
        clean = attn_operands(call, V, N_SRC, H, D, h, seed=F + 3)
        ops = dict(clean)
        for name in ("k", "v") if call == "dot" else ("xs",):
            grown = np.concatenate([clean[name], np.zeros((1, F), np.float32)])      # a row behind the last id
            grown[0], grown[N_SRC] = np.nan, np.nan
            ops[name] = grown
        ops[ROWWISE[call]] = clean[ROWWISE[call]].copy()
        ops[ROWWISE[call]][EMPTY] = np.nan
        for dt in (F32, B16):
            what = tags(call, H, D, dt, "NaN rows that nothing names")
            y_clean = run_both_y(call, agg, clean, H, dt, what + " (clean)")
            y = run_both_y(call, agg, ops, H, dt, what)
            assert np.isfinite(y).all() and same_bits(y, y_clean), "%s: differs from the clean run" % what


# ------------------------------------------------------------------------------------------ e. the element-wise load path
def offset_view(x, lead, dt):
    """x's values in a dense view that starts `lead` elements into its buffer"""
    n, F = x.shape
    buf = torch.zeros(lead + n * F + 2, device=DEV, dtype=dt)
    view = buf[lead:lead + n * F].view(n, F)
    view.copy_(x)
    return view


@pytest.mark.parametrize("H,D", [(8, 16), (4, 128), (8, 128), (2, 301)])
def test_unaligned_and_pitched_views_give_the_bits_of_the_aligned_run(H, D):
    F, h = H * D, head_of(H)
    mask = mask_edges(PTR, ("first", 4))
    for call in CALLS:
        idx, clean, masked = masked_case(call, PTR, IDX, N_SRC, H, D, h, mask, seed=F + 4)
        nan_case = dict(clean)
        nan_case[SCORED[call]] = clean[SCORED[call]].copy()
        nan_case[SCORED[call]][idx[PTR[1:][DEG > 0] - 1][::2], h * D] = np.nan      # the last source of every second row with edges
        agg = gnc.Aggregator_GAT(dev(PTR), dev(idx), F, F)
        for ops, name in ((masked, "masked"), (nan_case, "NaN")):
            for dt in (F32, B16):
                what = tags(call, H, D, dt, name)
                t = on_device(call, ops, dt)
                if geometry(F, H, t[SCORED[call]].element_size())["segred"]:
                    assert all(t[k].data_ptr() % 16 == 0 for k in t if k != "a")
                for ydt in (F32, B16):
                    y = full((V, F), ydt)
                    launch(call, agg, t, H, y)
                    want = np_of(y)
                    assert np.isnan(want).any() and np.isfinite(want).any()
                    if call == "dot":
                        (_, vq), (_, vk), (_, vv) = pitched(t["q"], F + 3, 1, dt), pitched(t["k"], F + 1, 3, dt), pitched(t["v"], F + 1, 5, dt)
                        assert all(x.data_ptr() % 16 != 0 for x in (vq, vk, vv))
                        y1 = full((V, F), ydt)
                        agg.run_dot(vq, vk, vv, y1, heads=H)
                        qpad = torch.zeros((N_SRC, F), device=DEV, dtype=dt)
                        qpad[:V] = t["q"]
                        packed = torch.cat([qpad, t["k"], t["v"]], dim=1)
                        y2 = full((V, F), ydt)
                        agg.run_dot(packed[:, :F], packed[:, F:2 * F], packed[:, 2 * F:], y2, heads=H)
                        odd = offset_view(packed, 1, dt)
                        y3 = full((V, F), ydt)
                        agg.run_dot(odd[:, :F], odd[:, F:2 * F], odd[:, 2 * F:], y3, heads=H)
                        got = (y1, y2, y3)
                    else:
                        vs, vd = offset_view(t["xs"], 1, dt), offset_view(t["xd"], 3, dt)
                        assert vs.data_ptr() % 16 != 0 and vd.data_ptr() % 16 != 0
                        y1 = full((V, F), ydt)
                        agg.run_v2(vs, vd, t["a"], y1, heads=H, slope=SLOPE)
                        got = (y1,)
                    for n, g in enumerate(got):
                        assert same_bits(np_of(g), want), "%s, %s y, view %d: not the bits of the aligned run" % (what, ydt, n)
