"""Host: the generators and judges of tests/test_gpu_gat_logits.py, pinned against the C oracle without a GPU.

The GAT kernels form w_e = expf(leaky_relu(att[dst, h, 0] + att[src, h, 1])) in fp32 without subtracting a row maximum, as the reference
does (aggr_gat.h:138-143): a trained model reaches weights of 1e+-30, +Inf (leaky logit above 88.73) and exact +0 (below -103.98).  The
regimes generated here:

  wide       a_dst ~ U[-30, 30], a_src ~ U[-320, 40] (U[-40, 40] at slope 1.0): leaky logits in [-70, 70], weights in about
             [4e-31, 3e30], all normal, and no sum of 4000 terms w |x| overflows.  Judge: the suite's bound 1e-5 (gat_scale + |ref|).
  overflow   the source term of a few sources, or the destination term of a few rows, of ONE head set to 100.0, +Inf or NaN: the weight
             is +Inf (NaN), the head's columns of exactly the rows concerned are NaN.
  underflow  the same places set to -700.0 (leaky logit <= -130: expf gives +0 exactly) or -Inf: a zero weight is an exact no-op in every
             chain, and a (row, head) whose weights are all zero has the denominator 0.

Deliberately NOT generated: the band of denormal weights (leaky logit in about [-104, -87]) and the last ulps below the overflow
threshold.  A relative bound means nothing on a denormal (its own rounding error is up to 100 %), and at either threshold one ulp of expf
-- device and libm may differ by that -- moves the weight into another class, so no class map could be asserted.

gat_ref_w32 is the judge of the class maps: the weights as fp32 numpy forms them (overflow and underflow included), everything after
that in float64; a zero denominator is divided like any other (NaN, aggr_gat.h:163).  The oracle's two restatements differ exactly there:
orc.gat_fused divides unguarded (NaN), orc.gat_grouped divides where the denominator is non-zero (the un-divided numerator, +0 for
finite features; scaleArray, aggr_gat.h:207-213).  This file pins both."""
import numpy as np
import pytest

import gnn_computing_amd as gnc
from oracle import oracle as orc
from test_nonfinite_host import (FINITE, INF, NAN, _per_row, assert_same_classes, classes, gat_hub_graph, hub_last_source, nan_sources,
                                 powerlaw, rand, reached)

RTOL = 1e-5
SLOPES = (0.2, 0.01, 1.0)
OVERFLOW = (100.0, INF, float("nan"))
UNDERFLOW = (-700.0, -INF)
SRC, DST = 1, 0          # att[v, h, 1]: the term of v as a source; att[v, h, 0]: the term of v as a destination row


def plus_zero(a):
    return bool(np.all(a == 0)) and not np.signbit(a).any()


def same(a, b):
    """bit-for-bit as values, NaN equal to NaN"""
    return np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------ the reference
def edge_weights32(ptr, idx, att, heads=1, slope=0.2):
    """[E, H] float32: exp(max(s, s * slope)) formed in fp32 like edge_weight() of kernel_util.cuh: +Inf above the overflow threshold, +0
    below the underflow threshold, NaN from a NaN term"""
    V = len(ptr) - 1
    rows = np.repeat(np.arange(V), np.diff(ptr))
    a = np.ascontiguousarray(att, dtype=np.float32).reshape(V, heads, 2)
    with np.errstate(all="ignore"):
        s = a[rows, :, 0] + a[idx, :, 1]
        l = s * np.float32(slope)
        w = np.exp(np.where(s > l, s, l))
    assert s.dtype == np.float32 and l.dtype == np.float32 and w.dtype == np.float32
    return w


def gat_ref_w32(ptr, idx, att, x, heads=1, slope=0.2, block=16):
    """(y [V, F] float64, w [E, H] float32): y = sum_e w_e x_e / sum_e w_e per head in float64 over the fp32 weights; rows without edges
    are 0, a zero denominator is divided like any other (NaN)"""
    V, F = len(ptr) - 1, x.shape[1]
    D = F // heads
    w = edge_weights32(ptr, idx, att, heads, slope)
    wt = np.ascontiguousarray(w.T, dtype=np.float64)                       # [H, E]
    xt = np.ascontiguousarray(x.T, dtype=np.float64)
    out = np.zeros((F, V))
    nz = np.diff(ptr) > 0
    with np.errstate(all="ignore"):
        den = _per_row(np.add, ptr, wt, 0.0)                               # [H, V]
        for c0 in range(0, F, block):
            heads_of = np.arange(c0, min(c0 + block, F)) // D
            num = _per_row(np.add, ptr, np.take(xt[c0:c0 + block], idx, axis=1) * wt[heads_of], 0.0)
            out[c0:c0 + block][:, nz] = num[:, nz] / den[heads_of][:, nz]
    return np.ascontiguousarray(out.T), w


def zero_denominators(ptr, w):
    """bool [V, H]: (row, head)s that have edges and whose weights are all +0"""
    V = len(ptr) - 1
    den = _per_row(np.add, ptr, np.ascontiguousarray(w.T, dtype=np.float64), 0.0).T
    return (den == 0) & (np.diff(ptr) > 0)[:, None]


def gat_scale(ptr, idx, att, x, heads, slope=0.2, block=16):
    """tests/test_gpu_parity.py::gat_scale -- sum_e w_e |x_e| / sum_e w_e with the oracle's normalised fp32 weights, float64 sums, stored
    as float32 -- through reduceat over column blocks instead of np.add.at over an [E, F] array (seconds on the dense test graphs)"""
    V, F = len(ptr) - 1, x.shape[1]
    D = F // heads
    with np.errstate(all="ignore"):
        wt = np.ascontiguousarray(orc.gat_att(ptr, idx, att, heads, slope).T, dtype=np.float64)
        xt = np.abs(np.ascontiguousarray(x.T, dtype=np.float64))
        out = np.zeros((F, V))
        for c0 in range(0, F, block):
            heads_of = np.arange(c0, min(c0 + block, F)) // D
            out[c0:c0 + block] = _per_row(np.add, ptr, np.take(xt[c0:c0 + block], idx, axis=1) * wt[heads_of], 0.0)
        return np.ascontiguousarray(out.T).astype(np.float32)


def worst_ratio(y, ref, scale, where=None):
    """max over the elements (of `where`) of |y - ref| / (1e-5 scale + 1e-30): the bound of test_gpu_parity.py::assert_within holds where
    this is <= 1"""
    with np.errstate(all="ignore"):
        r = np.abs(y.astype(np.float64) - ref.astype(np.float64)) / (RTOL * scale.astype(np.float64) + 1e-30)
    if where is not None:
        r = r[where]
    assert not np.isnan(r).any(), "a NaN among the elements to compare"
    return float(r.max()) if r.size else 0.0


def sources_range(ptr, idx, x, block=16):
    """(lo, hi) [V, F] float64: per row and column the smallest and largest feature value among the row's sources (0, 0 without edges):
    a softmax-weighted mean is a convex combination of them"""
    V, F = len(ptr) - 1, x.shape[1]
    xt = np.ascontiguousarray(x.T, dtype=np.float64)
    lo, hi = np.zeros((F, V)), np.zeros((F, V))
    nz = np.diff(ptr) > 0
    for c0 in range(0, F, block):
        g = np.take(xt[c0:c0 + block], idx, axis=1)
        lo[c0:c0 + block][:, nz] = _per_row(np.minimum, ptr, g, np.inf)[:, nz]
        hi[c0:c0 + block][:, nz] = _per_row(np.maximum, ptr, g, -np.inf)[:, nz]
    return np.ascontiguousarray(lo.T), np.ascontiguousarray(hi.T)


# ------------------------------------------------------------------------------------------------ the generators
def wide_att(V, H, slope, seed):
    """the wide regime for `slope` (one of SLOPES): every leaky logit in [-70, 70]"""
    assert slope in SLOPES
    rng = np.random.default_rng(seed)
    att = np.empty((V, H, 2), np.float32)
    att[:, :, DST] = rng.uniform(-30.0, 30.0, (V, H))
    att[:, :, SRC] = rng.uniform(-40.0 if slope == 1.0 else -320.0, 40.0, (V, H))
    return att


def poisoned(att, where, nodes, h, value):
    """a copy of att [V, H, 2] with att[nodes, h, where] = value"""
    a = np.array(att, dtype=np.float32, copy=True)
    a[np.atleast_1d(nodes), h, where] = value
    return a


def touched_rows(ptr, idx, where, nodes):
    """bool [V]: rows WITH EDGES that att[nodes, ., where] reaches: the rows that have one of `nodes` as a neighbor / the rows `nodes`"""
    V = len(ptr) - 1
    if where == SRC:
        return reached(ptr, idx, nodes)
    hit = np.zeros(V, bool)
    hit[np.atleast_1d(nodes)] = True
    return hit & (np.diff(ptr) > 0)


def touched_edges(ptr, idx, where, nodes):
    """bool [E]: the edges whose weight att[nodes, ., where] enters"""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return np.isin(idx if where == SRC else rows, np.atleast_1d(nodes))


def captive_rows(ptr, idx, sources):
    """bool [V]: rows with edges whose sources ALL lie in `sources`: a zero weight in every source leaves them the denominator 0"""
    V = len(ptr) - 1
    rows = np.repeat(np.arange(V), np.diff(ptr))
    free = np.zeros(V, bool)
    free[rows[~np.isin(idx, np.atleast_1d(sources))]] = True
    return ~free & (np.diff(ptr) > 0)


def poison_sources(ptr, idx, n):
    """Source nodes that together reach at least 8 and at most half of the rows: nan_sources(ptr, idx, n) plus the source of the longest
    row's last edge (where the clamps of a ragged last round point); picks of nan_sources are dropped from the end while the union
    reaches more than half of the rows."""
    V = len(ptr) - 1
    hs = hub_last_source(ptr, idx)
    s = [v for v in nan_sources(ptr, idx, n) if v != hs]
    while s and reached(ptr, idx, s + [hs]).sum() > V // 2:
        s.pop()
    s.append(hs)
    hit = reached(ptr, idx, s).sum()
    assert 8 <= hit <= V // 2, (s, int(hit), V)
    return s


def poison_rows(ptr):
    """Destination rows: the longest row, one row of 128 ... 1023 edges (above the lane-group class, below the hub threshold of the rows
    mode), one row of 1 ... 4 edges and one row without edges (it must stay +0) -- each where the graph has one."""
    deg = np.diff(ptr)
    out = [int(np.argmax(deg))]
    for lo, hi in ((128, 1023), (1, 4), (0, 0)):
        c = np.flatnonzero((deg >= lo) & (deg <= hi))
        c = c[~np.isin(c, out)]
        if len(c):
            out.append(int(c[np.argmax(deg[c])]))
    return out


def with_probe_rows(ptr, idx, sources):
    """(ptr, idx) with a row of one edge, from sources[0], appended when no row has all its sources in `sources` (a zero denominator from
    the source side), and a row without edges appended when the graph has none.  The appended rows are nobody's source."""
    ptr, idx = np.asarray(ptr, np.int32), np.asarray(idx, np.int32)
    if not captive_rows(ptr, idx, sources).any():
        ptr, idx = np.append(ptr, ptr[-1] + 1).astype(np.int32), np.append(idx, sources[0]).astype(np.int32)
    if (np.diff(ptr) > 0).all():
        ptr = np.append(ptr, ptr[-1]).astype(np.int32)
    return ptr, idx


_graphs = {}


def logit_graph(name):
    """(ptr, idx, poison sources, poison rows) of the graphs of tests/test_gpu_nonfinite.py, with the probe rows; made once"""
    if name not in _graphs:
        ptr, idx = {"powerlaw": lambda: powerlaw(3000, 120000, 5, 1.1), "blocked": lambda: powerlaw(900, 260000, 5, 0.9),
                    "bf16": lambda: powerlaw(4000, 100000, 9, 1.1), "gat_hubs": gat_hub_graph, "softmax_hubs": softmax_hub_graph,
                    "items": items_graph, "host": host_graph}[name]()
        s = poison_sources(ptr, idx, 1 if name == "blocked" else 5)
        ptr, idx = with_probe_rows(ptr, idx, s)
        assert poison_sources(ptr, idx, 1 if name == "blocked" else 5) == s
        _graphs[name] = (ptr, idx, s, poison_rows(ptr))
    return _graphs[name]


def softmax_hub_graph():
    """the graph of test_gpu_parity.py::test_edge_softmax_kernels_with_hub_rows"""
    V = 400
    rng = np.random.default_rng(9)
    deg = rng.integers(0, 5, V)
    deg[3], deg[200] = 3000, 700
    ptr = np.zeros(V + 1, np.int32)
    ptr[1:] = np.cumsum(deg)
    return ptr, rng.integers(0, V, int(ptr[-1])).astype(np.int32)


def items_graph():
    """600 rows of 0 ... 8 edges, a hub of 1500 and a row of 200: with a neighbor grouping of 2 most rows are 2 ... 4 groups, which the
    library runs on the one-item-per-lane-group kernels + k_combine rather than on the plan kernel (do_schedule, api.hip)"""
    V = 600
    rng = np.random.default_rng(37)
    deg = rng.integers(0, 9, V)
    deg[5], deg[300] = 1500, 200
    ptr = np.zeros(V + 1, np.int32)
    ptr[1:] = np.cumsum(deg)
    return ptr, rng.integers(0, V, int(ptr[-1])).astype(np.int32)


def host_graph():
    """400 rows of 0 ... 6 edges, a hub of 2500 and a row of 300"""
    V = 400
    rng = np.random.default_rng(31)
    deg = rng.integers(0, 7, V)
    deg[7], deg[250] = 2500, 300
    ptr = np.zeros(V + 1, np.int32)
    ptr[1:] = np.cumsum(deg)
    return ptr, rng.integers(0, V, int(ptr[-1])).astype(np.int32)


def poison_cases(name, H, values):
    """[(what, where, nodes, head, value)]: every value at the source terms of the poison sources and at the destination terms of the
    poison rows, in the one head H // 2 (not head 0 where H > 1: ordinary heads on both sides from H = 3 on)"""
    _, _, s, r = logit_graph(name)
    h = H // 2
    return [("att[%s, %d, %d] = %s" % (nodes, h, where, v), where, nodes, h, v) for v in values for where, nodes in ((SRC, s), (DST, r))]


def head_columns(F, H, h):
    D = F // H
    return np.arange(h * D, (h + 1) * D)


# ------------------------------------------------------------------------------------------------ the tests
def test_thresholds_of_numpy_and_the_oracle():
    with np.errstate(over="ignore", under="ignore"):
        assert np.exp(np.float32(95)) == np.inf and np.exp(np.float32(-130)) == 0 and not np.signbit(np.exp(np.float32(-130)))
        assert np.isfinite(np.exp(np.float32(70))) and np.exp(np.float32(-70)) > np.finfo(np.float32).tiny
    ptr, idx = np.array([0, 3, 3], np.int32), np.array([0, 1, 0], np.int32)       # row 0: sources 0, 1, 0; row 1: no edges
    x = np.array([[1.0], [2.0]], np.float32)
    for slope, up, down in ((0.2, 95.0, -700.0), (1.0, 95.0, -130.0), (0.01, 95.0, -13000.0)):
        for v, w1 in ((up, np.inf), (down, 0.0)):
            att = np.zeros((2, 1, 2), np.float32)
            att[1, 0, SRC] = v
            w = edge_weights32(ptr, idx, att, 1, slope)
            assert w[:, 0].tolist() == [1.0, w1, 1.0] and not np.signbit(w).any()
            _, nv, den = orc.gat_grouped(*orc.neighbor_grouping(ptr, 16), idx, att, x, 2, 1, slope)
            assert same(nv, w) and not np.signbit(nv).any() and den[0, 0] == 2.0 + w1
            soft = orc.gat_att(ptr, idx, att, 1, slope)[:, 0]
            if v == up:      # w / sum unguarded (attGat): NaN at the Inf edge, +0 at the finite edges of the row
                assert np.isnan(soft[1]) and plus_zero(soft[[0, 2]])
            else:
                assert soft.tolist() == [0.5, 0.0, 0.5] and not np.signbit(soft).any()
    # every weight of a (row, head) zero: attGat's 0 / 0 on every edge
    att = np.zeros((2, 1, 2), np.float32)
    att[0, 0, DST] = -700.0
    assert np.isnan(orc.gat_att(ptr, idx, att, 1, 0.2)).all()


@pytest.mark.parametrize("slope", SLOPES)
def test_wide_regime_stays_normal(slope):
    for name in ("host", "gat_hubs", "powerlaw"):
        ptr, idx, _, _ = logit_graph(name)
        V = len(ptr) - 1
        for H in (1, 3):
            w = edge_weights32(ptr, idx, wide_att(V, H, slope, 3), H, slope)
            assert np.isfinite(w).all() and w.min() >= 3e-31 and w.max() <= 3e30, (name, H, float(w.min()), float(w.max()))
            # 4000 terms w |x| with |x| < 6 (randn, fp32) stay far below FLT_MAX
            assert float(w.max()) * 4000 * 6 < 1e-3 * np.finfo(np.float32).max
    if slope != 1.0:
        assert float(w.max()) / float(w.min()) > 1e20       # (and the regime IS wide)


def test_gat_scale_is_the_suites():
    ptr, idx, _, _ = logit_graph("host")
    V, F, H = len(ptr) - 1, 12, 3
    x, att = rand((V, F), 1), wide_att(V, H, 0.2, 2)
    w = orc.gat_att(ptr, idx, att, H, 0.2)
    s = np.zeros((V, F))
    np.add.at(s, np.repeat(np.arange(V), np.diff(ptr)), np.repeat(w, F // H, axis=1).astype(np.float64) * np.abs(x[idx]))   # (gat_scale)
    np.testing.assert_allclose(gat_scale(ptr, idx, att, x, H), s.astype(np.float32), rtol=1e-6, atol=0)


@pytest.mark.parametrize("slope", SLOPES)
def test_oracles_stay_within_the_bound_of_the_float64_reference_on_wide_logits(slope):
    """measured worst ratios |oracle - ref| / (1e-5 (gat_scale + |ref|)): 0.01 ... 0.28 (printed with -s)"""
    ptr, idx, _, _ = logit_graph("host")
    V = len(ptr) - 1
    assert int(np.diff(ptr).max()) == 2500
    ps, tg = orc.neighbor_grouping(ptr, 16)
    for F, H in ((30, 3), (64, 1)):
        x, att = rand((V, F), 1), wide_att(V, H, slope, 2)
        ref, w = gat_ref_w32(ptr, idx, att, x, H, slope)
        assert np.isfinite(ref).all() and np.isfinite(w).all() and (w > 0).all()
        bound = gat_scale(ptr, idx, att, x, H, slope) + np.abs(ref)
        lo, hi = sources_range(ptr, idx, x)
        assert (ref >= lo - 1e-9).all() and (ref <= hi + 1e-9).all()        # a convex combination
        for what, y in (("gat_fused", orc.gat_fused(ptr, idx, att, x, H, slope)),
                        ("gat_grouped", orc.gat_grouped(ps, tg, idx, att, x, V, H, slope, seg=16)[0])):
            ratio = worst_ratio(y, ref, bound)
            print("slope %g F=%d H=%d %s: worst ratio %.3g" % (slope, F, H, what, ratio))
            assert ratio < 1, "%s, slope %g, F=%d H=%d: worst ratio %.3g of the bound" % (what, slope, F, H, ratio)
            assert plus_zero(y[np.diff(ptr) == 0])
        nv = orc.gat_grouped(ps, tg, idx, att, x, V, H, slope, seg=16)[1]
        np.testing.assert_allclose(nv, w, rtol=1e-5, atol=0)


@pytest.mark.parametrize("name,n", [("powerlaw", 5), ("blocked", 1), ("bf16", 5), ("gat_hubs", 5), ("softmax_hubs", 5), ("items", 5), ("host", 5)])
def test_poison_sources_and_rows(name, n):
    ptr, idx, s, r = logit_graph(name)
    V, deg = len(ptr) - 1, np.diff(ptr)
    hit = reached(ptr, idx, s)
    assert 1 <= len(s) <= n + 1 and len(set(s)) == len(s) and 8 <= hit.sum() <= V // 2
    assert s[-1] == hub_last_source(ptr, idx) and hit[int(np.argmax(deg))]
    cap = captive_rows(ptr, idx, s)
    assert cap.any() and (cap <= hit).all() and not cap.all()
    for row in np.flatnonzero(cap)[:5]:
        assert np.isin(idx[ptr[row]:ptr[row + 1]], s).all()
    # the destination rows: the longest, a medium one where the graph has one, a short one, one without edges
    assert r[0] == int(np.argmax(deg)) and len(set(r)) == len(r)
    d = deg[r].tolist()
    assert d[-1] == 0 and 1 <= d[-2] <= 4 and (len(r) == 3 or 128 <= d[1] <= 1023), d
    assert (len(r) == 4) == bool(((deg >= 128) & (deg <= 1023) & (np.arange(V) != r[0])).any())
    assert touched_rows(ptr, idx, DST, r).sum() == len(r) - 1 and touched_edges(ptr, idx, DST, r).sum() == deg[r].sum()
    assert np.array_equal(touched_rows(ptr, idx, SRC, s), hit) and touched_edges(ptr, idx, SRC, s).sum() == np.isin(idx, s).sum()


@pytest.mark.parametrize("F,H", [(30, 3), (64, 1), (32, 8)])
def test_oracles_on_the_poison_cases(F, H):
    ptr, idx, s, r = logit_graph("host")
    V, deg = len(ptr) - 1, np.diff(ptr)
    D = F // H
    x, att = rand((V, F), 1), rand((V, H, 2), 2) * np.float32(0.4)
    ps, tg = orc.neighbor_grouping(ptr, 16)
    fused_clean = orc.gat_fused(ptr, idx, att, x, H)
    grouped_clean, nv_clean, _ = orc.gat_grouped(ps, tg, idx, att, x, V, H, seg=16)
    assert np.isfinite(fused_clean).all() and np.isfinite(grouped_clean).all()
    seen_zero_den = {SRC: 0, DST: 0}
    for what, where, nodes, h, v in poison_cases("host", H, OVERFLOW + UNDERFLOW):
        assert h != 0 or H == 1
        pa = poisoned(att, where, nodes, h, v)
        ref, w = gat_ref_w32(ptr, idx, pa, x, H)
        fused = orc.gat_fused(ptr, idx, pa, x, H)
        grouped, nv, _ = orc.gat_grouped(ps, tg, idx, pa, x, V, H, seg=16)
        rows_hit, edges_hit = touched_rows(ptr, idx, where, nodes), touched_edges(ptr, idx, where, nodes)
        cols = head_columns(F, H, h)
        other = np.setdiff1d(np.arange(F), cols)
        zd = zero_denominators(ptr, w)
        zd_el = np.repeat(zd, D, axis=1)
        # the class map of the reference everywhere but at the zero denominators; there NaN (fused) / +0 (grouped)
        assert np.isnan(ref[zd_el]).all()
        for name, y in (("gat_fused", fused), ("gat_grouped", grouped)):
            assert_same_classes(np.where(zd_el, np.nan, y), ref, "%s, %s" % (name, what))
            assert plus_zero(y[deg == 0]), what
        assert np.isnan(fused[zd_el]).all() and plus_zero(grouped[zd_el]), what
        # locality: the other heads, and the head's columns of the other rows, are the clean run's bits
        for y, clean in ((fused, fused_clean), (grouped, grouped_clean)):
            assert np.array_equal(y[:, other], clean[:, other]) and np.array_equal(y[~rows_hit][:, cols], clean[~rows_hit][:, cols]), what
        assert np.array_equal(np.delete(nv, h, 1), np.delete(nv_clean, h, 1)) and np.array_equal(nv[~edges_hit, h], nv_clean[~edges_hit, h])
        assert np.allclose(nv, w, rtol=1e-6, atol=0, equal_nan=True), what      # (libm's expf and numpy's differ by an ulp)
        if v in UNDERFLOW:
            assert plus_zero(nv[edges_hit, h]) and np.array_equal(zd.any(axis=1), zd[:, h]), what
            want = captive_rows(ptr, idx, nodes) if where == SRC else rows_hit
            assert np.array_equal(zd[:, h], want), what
            seen_zero_den[where] += int(zd.sum())
            live = rows_hit & ~zd[:, h]
            assert np.isfinite(fused[live][:, cols]).all() and np.isfinite(grouped[live][:, cols]).all(), what
        else:
            assert not zd.any()
            assert (np.isnan(nv[edges_hit, h]).all() if v != v else np.isposinf(nv[edges_hit, h]).all()), what
            assert np.isnan(ref[rows_hit][:, cols]).all() and np.isfinite(ref[~rows_hit]).all(), what
            assert (classes(ref) == NAN).sum() == rows_hit.sum() * D and set(np.unique(classes(ref)).tolist()) == {FINITE, NAN}
    assert seen_zero_den[SRC] > 0 and seen_zero_den[DST] > 0
