"""GPU: gnnagg_gcn_run_multi (Aggregator_GCN.run_multi) on non-finite messages, on the fixture graph of tests/test_multi_aggr_host.py.

The contract (include/gnnagg.h, "non-finite" under gnnagg_gcn_run_multi), judged per run by `judge`:
  * sum, mean, var, std: the class map (finite / +Inf / -Inf / NaN) of the float64 two-moment reference multi_ref_nf -- var and std NaN
    wherever a message of the (row, column) is +-Inf or NaN;
  * min, max: NaN messages skipped, +-Inf exact (== the reference wherever it is not NaN), NaN where every message is NaN;
  * every (row, column) no non-finite message reaches: the bits of the run without the poison; rows without edges +0.
The inputs are the themes of tests/test_multi_aggr_nonfinite_host.py, which checks the generators and the reference on the host."""
import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from test_multi_aggr_host import AGGRS, CENSUS_BF16, LONG_EDGES, SCALERS, SEG_EDGES, fixture_graph, messages32, multi_layout, multi_width
from test_multi_aggr_nonfinite_host import (INF, NF_F, QNAN, ROW_1100, all_themes, multi_ref_nf, nf_val, nf_x, reach_map, theme_all_nan,
                                            theme_positions, theme_sources, theme_zero_times_inf)
from test_nonfinite_host import assert_same_classes, classes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
PTR, IDX, N_SRC = fixture_graph()
V, E = len(PTR) - 1, len(IDX)
DEG = np.diff(PTR)
SHORT, HAS = DEG <= LONG_EDGES, DEG > 0
DELTA = gnc.pna_delta(PTR)
IDENT = ("identity",)


def dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)   # (a copy: the cached inputs of the host file are read-only)


def handle(c):
    return gnc.Aggregator_GCN(dev(PTR), dev(c["idx"]), None if c["val"] is None else dev(c["val"]))


def run(at, x, aggrs=AGGRS, scalers=IDENT, ydtype=torch.float32):
    x = x if isinstance(x, torch.Tensor) else dev(x)
    y = torch.full((V, multi_width(aggrs, scalers, x.shape[1])), 7.0, device=DEV, dtype=ydtype)
    at.run_multi(x, y, aggrs=aggrs, scalers=scalers, delta=DELTA)
    return y


def blocks(y, aggrs, scalers, F):
    a = y.float().cpu().numpy() if y.dtype == BF else y.cpu().numpy()
    return {k: a[:, s] for k, s in multi_layout(aggrs, scalers, F).items()}


def np_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32),
                                                                          b.view(torch.int16 if b.dtype == BF else torch.int32)))


def run_case(c, aggrs=AGGRS, scalers=IDENT):
    """(poisoned run, clean run) of one case of a theme, on one handle: the edge values are replaced as a caller would"""
    at = handle(c)
    got = run(at, c["x"], aggrs, scalers)
    if c["clean_val"] is not None and c["clean_val"] is not c["val"]:
        at.updateval(dev(c["clean_val"]))
    clean = run(at, c["clean_x"], aggrs, scalers)
    assert bool(torch.isfinite(clean).all()), c["label"]
    return got, clean


def judge(got, clean, c, F, scaler="identity", scalers=IDENT):
    """the identity (or `scaler`) blocks of a fp32-y run against the contract"""
    ref = multi_ref_nf(PTR, c["idx"], c["val"], c["x"])
    reach = reach_map(PTR, c["idx"], c["val"], c["x"])
    g, cl = blocks(got, AGGRS, scalers, F), blocks(clean, AGGRS, scalers, F)
    for k in AGGRS:
        what = "%s, F = %d, %s" % (c["label"], F, k)
        assert_same_classes(g[(scaler, k)], ref[k], what)
        assert np.array_equal(np_bits(g[(scaler, k)])[~reach], np_bits(cl[(scaler, k)])[~reach]), what + ": a value changed that nothing non-finite reaches"
        assert not np_bits(g[(scaler, k)][~HAS]).any(), what + ": a row without edges is not +0"
    for k in ("min", "max"):
        keep = ~np.isnan(ref[k])
        assert np.array_equal(g[("identity", k)][keep].astype(np.float64), ref[k][keep]), "%s, F = %d: %s is not the extremum of the other messages" % (
            c["label"], F, k)
    return g, ref, reach


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", NF_F)
@pytest.mark.parametrize("with_val", [False, True])
def test_whole_source_poison(F, with_val):
    for c in theme_sources(F, with_val):
        got, clean = run_case(c)
        g, ref, reach = judge(got, clean, c, F)
        assert reach.any() and (~reach[HAS]).any()
        assert np.isnan(g[("identity", "var")][reach]).all() and np.isnan(g[("identity", "std")][reach]).all()


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", NF_F)
@pytest.mark.parametrize("value", [QNAN, INF], ids=["nan", "inf"])
def test_one_poisoned_edge_at_every_position_of_the_walk(F, value):
    """val[p] = NaN / +Inf at one edge per row per run: edge 0, the batch's last, the second lane group's first, either side of the segment
    boundary, the third segment, the row's last.  var and std are NaN, sum is +-Inf or NaN, min and max are the extrema of the other
    messages (NaN) or the infinity (Inf).  On the kernel before the NaN-keeping clamp this test failed at every width: var finite (0) where
    the reference is NaN (the +Inf runs), and -- min being judged before var -- the one-edge row's min = +Inf where it is NaN (the NaN runs)."""
    cases = theme_positions(F, value)
    at = handle(cases[0])
    clean = None
    for c in cases:
        at.updateval(dev(c["val"]))
        got = run(at, c["x"])
        if clean is None:
            at.updateval(dev(c["clean_val"]))
            clean = run(at, c["clean_x"])
            assert bool(torch.isfinite(clean).all())
        g, ref, reach = judge(got, clean, c, F)
        rows = reach.any(1)
        assert rows.any() and reach[rows].all()                      # a poisoned val reaches every column of its row
        assert np.isnan(g[("identity", "var")][rows]).all() and np.isnan(g[("identity", "std")][rows]).all()
        s = g[("identity", "sum")][rows]
        assert np.isnan(s).all() if np.isnan(value) else (np.isinf(s) | np.isnan(s)).all()


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", NF_F)
def test_all_nan_columns_and_segments(F):
    """a (row, column) whose messages are all NaN is NaN in min and max, never the +-Inf the chains start from: rows 513 and 1100 go through
    the scratch slots and the merge.  On the kernel before the fix the first two cases failed at every width: min = +Inf, max = -Inf."""
    col_novalue, col_val, seg = theme_all_nan(F)
    col = F // 3
    for c in (col_novalue, col_val):
        got, clean = run_case(c)
        g, ref, reach = judge(got, clean, c, F)
        assert np.isnan(g[("identity", "min")][HAS, col]).all() and np.isnan(g[("identity", "max")][HAS, col]).all()
        others = np.ones(F, bool)
        others[col] = False
        assert np.array_equal(reach, HAS[:, None] & ~others[None, :])
    got, clean = run_case(seg)
    g, ref, reach = judge(got, clean, seg, F)
    b = int(PTR[ROW_1100])
    keep = np.r_[b:b + SEG_EDGES, b + 2 * SEG_EDGES:b + 1100]
    m = messages32(IDX, seg["clean_val"], seg["x"])
    assert np.array_equal(g[("identity", "min")][ROW_1100], m[keep].min(0)) and np.array_equal(g[("identity", "max")][ROW_1100], m[keep].max(0))
    assert np.array_equal(reach.any(1), np.arange(V) == ROW_1100)


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", NF_F)
def test_zero_times_inf_is_formed_by_the_walk(F):
    c = theme_zero_times_inf(F)[0]
    got, clean = run_case(c)
    g, ref, reach = judge(got, clean, c, F)
    assert np.array_equal(reach, np.repeat(HAS[:, None], F, 1)) and np.isnan(g[("identity", "sum")][HAS]).all()
    assert np.isinf(g[("identity", "max")][HAS]).any()               # the edges that keep their value: an Inf message beside the NaN ones


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", NF_F)
def test_scaler_blocks_have_the_identity_blocks_classes(F):
    """deg > 0: the factors are finite and positive, so a scaled block has the class map of its aggregate; rows without edges stay +0"""
    for c in (theme_sources(F, True)[0], theme_positions(F, INF)[2], theme_all_nan(F)[1]):
        got, clean = run_case(c, scalers=SCALERS)
        for s in SCALERS:
            judge(got, clean, c, F, scaler=s, scalers=SCALERS)
        g = blocks(got, AGGRS, SCALERS, F)
        for s in ("amplification", "attenuation"):
            for k in AGGRS:
                assert np.array_equal(classes(g[(s, k)]), classes(g[("identity", k)])), (c["label"], s, k)


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [CENSUS_BF16[10801][0], CENSUS_BF16[6402][0], CENSUS_BF16[16401][0]])
def test_the_four_dtype_pairs_on_poisoned_input(F):
    assert F in (8, 100, 512)
    for c in (theme_sources(F, True)[0], theme_sources(F, False)[1], theme_all_nan(F)[1], theme_zero_times_inf(F)[0]):
        at = handle(c)
        xb = dev(c["x"]).to(BF)
        xw = xb.float()                                              # Inf and NaN survive the narrowing; what the bf16 call computes on
        y_ff, y_bf = run(at, xw, scalers=SCALERS), run(at, xb, scalers=SCALERS)
        short = dev(SHORT)
        assert same_bits(y_bf[short], y_ff[short]), c["label"] + ": bf16 x is not the fp32 call on the widened x (short rows)"
        assert np.array_equal(classes(y_bf.cpu().numpy()), classes(y_ff.cpu().numpy())), c["label"]
        cw = dict(c, x=xw.cpu().numpy())
        ref = multi_ref_nf(PTR, cw["idx"], cw["val"], cw["x"])
        g = blocks(y_bf, AGGRS, SCALERS, F)
        for k in AGGRS:
            assert_same_classes(g[("identity", k)], ref[k], "%s, bf16 x, F = %d, %s" % (c["label"], F, k))
        for x, y32 in ((xw, y_ff), (xb, y_bf)):
            y16, want = run(at, x, scalers=SCALERS, ydtype=BF), y32.to(BF)
            nan = torch.isnan(want)
            assert bool(torch.equal(torch.isnan(y16), nan)), c["label"] + ": a bf16 y lost or gained a NaN"
            assert same_bits(torch.where(nan, torch.zeros_like(y16), y16), torch.where(nan, torch.zeros_like(want), want)), \
                c["label"] + ": bf16 y is not one RNE rounding of the fp32 y"


# 7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", NF_F)
def test_the_four_template_arms_agree_on_poisoned_input(F):
    """min / max alone (the MM arm), var / std alone (S2), sum alone (neither) against the call with all six (both): the same bits, NaN
    payloads included -- the skip rule and the seeds are the same in every instantiation"""
    lay = multi_layout(AGGRS, IDENT, F)
    for c in (theme_positions(F, QNAN)[0], theme_positions(F, QNAN)[3], theme_positions(F, INF)[1], theme_all_nan(F)[1], theme_all_nan(F)[2],
              theme_zero_times_inf(F)[0], theme_sources(F, False)[0]):
        at = handle(c)
        x = dev(c["x"])
        full = run(at, x)
        for aggrs in (("min", "max"), ("var", "std"), ("sum",), ("mean",), ("min",), ("max", "std")):
            one = run(at, x, aggrs=aggrs)
            want = torch.cat([full[:, lay[("identity", a)]] for a in AGGRS if a in aggrs], 1)
            assert same_bits(one, want), (c["label"], aggrs)


def test_every_theme_of_the_host_file_is_run_here():
    """what the host file checks the restatement on (all_themes) is what tests 1 - 4 above run"""
    assert len(all_themes(5)) == 2 * len(theme_sources(5, True)) + len(theme_all_nan(5)) + len(theme_zero_times_inf(5)) + 2 * len(theme_positions(5, INF))
    assert nf_x(5).shape == (N_SRC, 5) and len(nf_val()) == E
