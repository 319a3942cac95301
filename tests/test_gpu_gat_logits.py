"""GPU: the GAT kernels over the whole range of attention logits (the contract of include/gnnagg.h, "Attention logits").

Every other GAT test draws att as 0.4 randn or 0.5 randn, so every edge weight exp(leaky(a_dst + a_src)) it ever produced lies in about
[0.1, 10], and none passes a slope other than 0.2.  edge_weight() (kernel_util.cuh) subtracts no maximum, as the reference: weights of
1e+-30, +Inf and exact +0 are ordinary inputs.  The regimes, generators and judges are those of tests/test_gat_logits_host.py:

  wide        leaky logits in [-70, 70], slopes 0.2 / 0.01 / 1.0: the suite's bound against the oracle that restates the form's order,
              newval within 1e-5, and -- needing no reference -- every output inside [min, max] of its own sources' features.
  overflow    100.0 / +Inf / NaN in the source term of a few sources, or the destination term of a few rows, of ONE head: that head's
              columns of exactly the rows concerned are NaN, newval holds the +Inf / NaN at exactly the edges concerned, and every other
              element of y and newval is the clean run's bit for bit -- a denominator read from the wrong head or the wrong row
              (partial_den[g H + h], den_t[..][HT], den_io[row H + h], the hub fold's LDS stage_den) is a class change here, not an error
              the 1e-5 bound absorbs.
  underflow   -700.0 / -Inf in the same places: zero weights are exact no-ops, and a (row, head) with edges whose denominator is 0 is
              NaN in the canonical order (rows, rows on the blocked order: aggr_gat's 0 / 0) and the un-divided numerator, +0, in every
              grouped order (scaleArray divides where the scalar is non-zero).

Every y and newval is prefilled with 7.0; every form asserts on the handle that it is the form meant."""
import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from oracle import oracle as orc
from test_gat_logits_host import (OVERFLOW, SLOPES, SRC, UNDERFLOW, captive_rows, edge_weights32, gat_ref_w32, gat_scale, head_columns,
                                  logit_graph, plus_zero, poison_cases, poison_sources, poisoned, same, sources_range, touched_edges,
                                  touched_rows, wide_att, worst_ratio, zero_denominators)
from test_gpu_blocked import _split_edges, hub_graph
from test_gpu_nonfinite import BF, same_t
from test_gpu_parity import DEV, dev, rand
from test_nonfinite_host import NAN, assert_same_classes, classes

pytestmark = pytest.mark.gpu

CANONICAL = ("rows_medium16", "rows_no_medium", "rows_blocked")          # a zero denominator is 0 / 0 = NaN; every other form: +0
GRAPH_OF = {"rows_medium16": "powerlaw", "rows_no_medium": "powerlaw", "scheduled32": "powerlaw", "scheduled2": "items",
            "balanced": "gat_hubs", "rows_blocked": "blocked", "blocked": "blocked", "blocked_tile32": "blocked", "blocked_tile128": "blocked"}
ALL_FH = [(128, 1), (256, 8), (96, 3), (30, 3)]
FORM_CASES = ([(f, F, H) for f in ("rows_medium16", "rows_no_medium", "scheduled32", "scheduled2", "balanced", "blocked") for F, H in ALL_FH] +
              [("rows_blocked", F, H) for F, H in ALL_FH[:3]] +          # (head width % 4 == 0: a quad of k_untile_y lies inside one head)
              [("blocked_tile32", 128, 1), ("blocked_tile32", 96, 3), ("blocked_tile128", 256, 8), ("blocked_tile128", 128, 1)])


class Form:
    """a GAT handle in one kernel form, the mode argument that reaches it, and the oracle that restates the order of its sums"""

    def __init__(self, form, F, H):
        self.form, self.F, self.H = form, F, H
        ptr, idx, self.s, self.r = logit_graph(GRAPH_OF[form])
        self.ptr, self.idx = ptr, idx
        self.V, self.E, self.deg = len(ptr) - 1, len(idx), np.diff(ptr)
        gat = self.gat = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
        self.newval_ok = form != "rows_blocked"                   # (a caller that asks for newval keeps the row kernels)
        self.groups = None
        if form in CANONICAL:
            self.m = 0
            gat.set_option("fast_rows", 0)
            if form == "rows_blocked":
                gat.set_option("slice_kb", 16)
            else:   # lane-group rows, 128-thread rows (16: every row above 16 edges; -1: no such class), the hub rows' long-row kernel
                gat.set_option("rows_blocked", 0)
                gat.set_option("rows_medium_edges", 16 if form == "rows_medium16" else -1)
                assert gat.rows_blocked_ranges() == 0 and gat.mode_params("rows") == (0x7fffffff, 0)
                assert self.deg.max() > max(1024, 16 * self.E // self.V) and ((self.deg > 128) & (self.deg < 1024)).any()
        elif form in ("scheduled32", "scheduled2"):
            self.m, ng = 1, int(form[9:])
            gat.set_option("fast_scheduled", 0)
            gat.schedule(gnc.Schedule.neighbor_grouping, [ng])
            assert gat.mode_params("scheduled") == (ng, 16 if ng == 32 else 0)      # the plan kernel / the item kernels + k_combine
            self.groups = orc.neighbor_grouping(ptr, ng) + (idx, gat.mode_params("scheduled")[1])
        elif form == "balanced":
            self.m = "balanced"
            gat.schedule_balanced(16)
            assert gat.balanced_partitions() == 0 and gat.balanced_params() == (16, 16) and self.deg.max() > 2 * 16 * 16
            self.groups = orc.neighbor_grouping(ptr, 16) + (idx, 16)
        else:
            self.m = "balanced"
            gat.set_option("slice_kb", 16)
            if form != "blocked":
                gat.set_option("tile_width", int(form[12:]))
            parts = gat.balanced_partitions()
            chunk, seg = gat.balanced_params()
            assert parts > 1 and seg == 0
            ps, ix, tg, _ = orc.locality_schedule(ptr, idx, parts, gat.balanced_partition_columns(), ng=chunk)
            self.groups = (ps, tg, ix, 0)

    def run(self, x, att, slope, with_newval):
        y = torch.full((self.V, self.F), 7.0, device=DEV)
        nv = torch.full((self.E, self.H), 7.0, device=DEV) if with_newval else None
        self.gat.run(x if isinstance(x, torch.Tensor) else dev(x), dev(att), y, 128, self.m, heads=self.H, slope=slope, newval=nv)
        if self.form == "rows_blocked" and not with_newval:
            assert self.gat.rows_blocked_ranges() > 1
        return y.cpu().numpy(), (None if nv is None else nv.cpu().numpy())

    def runs(self, x, att, slope=0.2):
        """[(y, newval or None)] with and without newval where the form has both"""
        return [self.run(x, att, slope, nv) for nv in ((True, False) if self.newval_ok else (False,))]

    def oracle(self, x, att, slope=0.2):
        """the same-order oracle the suite uses for this form: orc.gat_fused, or orc.gat_grouped over the form's groups"""
        if self.groups is None:
            return orc.gat_fused(self.ptr, self.idx, att, x, self.H, slope)
        ps, tg, ix, seg = self.groups
        return orc.gat_grouped(ps, tg, ix, att, x, self.V, self.H, slope, seg=seg)[0]


_forms, _data = {}, {}


def form_of(form, F, H):
    if (form, F, H) not in _forms:
        _forms[(form, F, H)] = Form(form, F, H)
    return _forms[(form, F, H)]


def shared(key, make):
    """references computed once and shared by the forms that run the same graph; never modified"""
    if key not in _data:
        _data[key] = make()
    return _data[key]


def features(gname, F):
    return shared(("x", gname, F), lambda: rand((len(logit_graph(gname)[0]) - 1, F), 1))


def base_att(gname, H):
    return shared(("att", gname, H), lambda: rand((len(logit_graph(gname)[0]) - 1, H, 2), 2) * np.float32(0.4))


def oracle_newval(ptr, idx, att, H, slope=0.2):
    """the un-normalised weights [E, H] in CSR edge order, by the oracle (one group per row; the features do not enter)"""
    V = len(ptr) - 1
    return orc.gat_grouped(*orc.neighbor_grouping(ptr, 1 << 30), idx, att, np.zeros((V, H), np.float32), V, H, slope)[1]


def ids(v):
    return repr(v) if isinstance(v, float) else str(v)


# ------------------------------------------------------------------------------------------------------------------ wide logits
@pytest.mark.parametrize("slope", SLOPES, ids=ids)
@pytest.mark.parametrize("form,F,H", FORM_CASES)
def test_wide_logits(form, F, H, slope):
    g = form_of(form, F, H)
    gname, ptr, idx = GRAPH_OF[form], g.ptr, g.idx
    x = features(gname, F)
    att = shared(("wide", gname, H, slope), lambda: wide_att(g.V, H, slope, 7))
    scale = shared(("wide scale", gname, F, H, slope), lambda: gat_scale(ptr, idx, att, x, H, slope))
    lo, hi = shared(("range", gname, F), lambda: sources_range(ptr, idx, x))
    ref_nv = shared(("wide newval", gname, H, slope), lambda: oracle_newval(ptr, idx, att, H, slope))
    ref = g.oracle(x, att, slope)
    assert np.isfinite(ref).all() and np.isfinite(ref_nv).all() and ref_nv.min() > 1e-31 and ref_nv.max() < 1e31
    bound = scale + np.abs(ref)
    for y, nv in g.runs(x, att, slope):
        what = "%s F=%d H=%d slope %g newval=%s" % (form, F, H, slope, nv is not None)
        ratio = worst_ratio(y, ref, bound)
        print("%s: worst ratio %.3g of 1e-5 (gat_scale + |ref|)" % (what, ratio))
        assert ratio <= 1, "%s: outside 1e-5 (gat_scale + |ref|) of the same-order oracle, worst ratio %.3g" % (what, ratio)
        assert plus_zero(y[g.deg == 0]), what
        # a softmax is a convex combination: whatever the reference says, y lies between its own sources' extremes
        tol = 1e-5 * bound.astype(np.float64) + 1e-30
        assert (y >= lo - tol).all() and (y <= hi + tol).all(), what + ": outside [min, max] of the row's own sources"
        if nv is not None:
            np.testing.assert_allclose(nv, ref_nv, rtol=1e-5, atol=0, err_msg=what)


# ------------------------------------------------------------------------------------------------------------------ poison
def clean_runs(g, gname):
    """(y, newval) of the form on the ordinary att, with newval where the form has it, and the bare y of the call without"""
    return shared(("clean", g.form, g.F, g.H), lambda: g.runs(features(gname, g.F), base_att(gname, g.H)))


@pytest.mark.parametrize("poison", OVERFLOW, ids=ids)
@pytest.mark.parametrize("form,F,H", FORM_CASES)
def test_overflow_is_confined(form, F, H, poison):
    g = form_of(form, F, H)
    gname, ptr, idx = GRAPH_OF[form], g.ptr, g.idx
    x, att = features(gname, F), base_att(gname, H)
    clean = clean_runs(g, gname)
    assert all(np.isfinite(y).all() for y, _ in clean)
    for what, where, nodes, h, v in poison_cases(gname, H, (poison,)):
        assert h != 0 or H == 1
        what = "%s F=%d H=%d, %s" % (form, F, H, what)
        pa = poisoned(att, where, nodes, h, v)
        ref_classes = shared(("overflow classes", gname, F, H, where, ids(v)), lambda: classes(gat_ref_w32(ptr, idx, pa, x, H)[0]))
        rows_hit, edges_hit = touched_rows(ptr, idx, where, nodes), touched_edges(ptr, idx, where, nodes)
        cols = head_columns(F, H, h)
        in_head = np.zeros(F, bool)
        in_head[cols] = True
        expect_nan = rows_hit[:, None] & in_head[None, :]
        assert np.array_equal(ref_classes == NAN, expect_nan) and not ref_classes[~expect_nan].any() and rows_hit.any()
        for (y, nv), (y_clean, nv_clean) in zip(g.runs(x, pa), clean):
            w = what + (", with newval" if nv is not None else "")
            assert np.array_equal(classes(y), ref_classes), w + ": not the class map of gat_ref_w32"
            assert np.isnan(y[expect_nan]).all(), w
            assert np.array_equal(y[~expect_nan], y_clean[~expect_nan]), w + ": an element outside the head of the rows concerned differs from the clean run"
            assert plus_zero(y[g.deg == 0]), w
            if nv is not None:
                hit = np.zeros(nv.shape, bool)
                hit[edges_hit, h] = True
                assert (np.isnan(nv[hit]).all() if v != v else np.isposinf(nv[hit]).all()), w + ": newval at the edges concerned"
                assert np.array_equal(nv[~hit], nv_clean[~hit]), w + ": newval elsewhere differs from the clean run"


@pytest.mark.parametrize("poison", UNDERFLOW, ids=ids)
@pytest.mark.parametrize("form,F,H", FORM_CASES)
def test_underflow(form, F, H, poison):
    g = form_of(form, F, H)
    gname, ptr, idx = GRAPH_OF[form], g.ptr, g.idx
    D = F // H
    x, att = features(gname, F), base_att(gname, H)
    clean = clean_runs(g, gname)
    seen = 0
    for what, where, nodes, h, v in poison_cases(gname, H, (poison,)):
        what = "%s F=%d H=%d, %s" % (form, F, H, what)
        pa = poisoned(att, where, nodes, h, v)
        wts = edge_weights32(ptr, idx, pa, H)
        rows_hit, edges_hit = touched_rows(ptr, idx, where, nodes), touched_edges(ptr, idx, where, nodes)
        zd = zero_denominators(ptr, wts)
        assert np.array_equal(zd[:, h], captive_rows(ptr, idx, nodes) if where == SRC else rows_hit) and zd.sum() == zd[:, h].sum() > 0
        assert plus_zero(wts[edges_hit, h]) and (wts[~edges_hit] > 0).all()
        seen += int(zd.sum())
        zd_el = np.repeat(zd, D, axis=1)
        in_head = np.zeros(F, bool)
        in_head[head_columns(F, H, h)] = True
        changed = rows_hit[:, None] & in_head[None, :]
        ref = g.oracle(x, pa)                      # (a zero weight is an exact no-op in the chain: the oracle as it is)
        bound = shared(("underflow scale", gname, F, H, where, ids(v)), lambda: gat_scale(ptr, idx, pa, x, H)) + np.abs(ref)
        assert np.isfinite(ref[~zd_el]).all()
        for (y, nv), (y_clean, nv_clean) in zip(g.runs(x, pa), clean):
            w = what + (", with newval" if nv is not None else "")
            # a (row, head) that keeps a non-zero weight
            assert np.isfinite(y[~zd_el]).all(), w
            ratio = worst_ratio(y, ref, bound, ~zd_el)
            assert ratio <= 1, "%s: outside the bound of the same-order oracle, worst ratio %.3g" % (w, ratio)
            # a (row, head) with edges and the denominator 0
            if form in CANONICAL:
                assert np.isnan(y[zd_el]).all(), w + ": a zero denominator in the canonical order is aggr_gat's 0 / 0 = NaN"
            else:
                assert plus_zero(y[zd_el]), w + ": a zero denominator in a grouped order leaves the un-divided numerator, +0"
            assert np.array_equal(y[~changed], y_clean[~changed]), w + ": an element outside the head of the rows concerned differs from the clean run"
            assert plus_zero(y[g.deg == 0]), w
            if nv is not None:
                hit = np.zeros(nv.shape, bool)
                hit[edges_hit, h] = True
                assert plus_zero(nv[hit]), w + ": newval of a zero-weight edge"
                assert np.array_equal(nv[~hit], nv_clean[~hit]), w + ": newval elsewhere differs from the clean run"
    assert seen > 0


@pytest.mark.parametrize("F,H", ALL_FH[:3])
def test_rows_blocked_equals_the_row_kernels_under_poison(F, H):
    """include/gnnagg.h, option "rows_blocked": "same bits either way" -- asserted where it can break: k_untile_y's division"""
    ptr, idx, s, r = logit_graph("blocked")
    V = len(ptr) - 1
    x, att = features("blocked", F), base_att("blocked", H)
    a, k = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F), gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    for h_ in (a, k):
        h_.set_option("fast_rows", 0)
        h_.set_option("slice_kb", 16)
    k.set_option("rows_blocked", 0)
    cases = [("clean", x, att), ("wide", x, wide_att(V, H, 0.2, 7))]
    cases += [(what, x, poisoned(att, where, nodes, h, v)) for what, where, nodes, h, v in poison_cases("blocked", H, OVERFLOW + UNDERFLOW)]
    # an Inf feature under a zero weight: 0 . Inf = NaN in the numerator, over a zero denominator in the rows that have no other source
    h = H // 2
    cases.append(("Inf features in the zero-weight sources", poison_inf_rows(x, s), poisoned(att, SRC, s, h, -700.0)))
    for what, xp, ap in cases:
        ya, yk = torch.full((V, F), 7.0, device=DEV), torch.full((V, F), 7.0, device=DEV)
        a.run(dev(xp), dev(ap), ya, 128, 0, heads=H)
        k.run(dev(xp), dev(ap), yk, 128, 0, heads=H)
        assert a.rows_blocked_ranges() > 1 and k.rows_blocked_ranges() == 0
        ya, yk = ya.cpu().numpy(), yk.cpu().numpy()
        bad = ~((ya == yk) | (np.isnan(ya) & np.isnan(yk)))
        assert not bad.any(), "%s: %d elements differ between the blocked order and the row kernels, first at %s: %r, row kernels %r" % (
            what, int(bad.sum()), tuple(np.argwhere(bad)[0]), ya[tuple(np.argwhere(bad)[0])], yk[tuple(np.argwhere(bad)[0])])
        if what.startswith("Inf features"):
            assert np.isnan(ya[touched_rows(ptr, idx, SRC, s)][:, head_columns(F, H, h)]).all()


def poison_inf_rows(x, sources):
    x = x.copy()
    x[np.atleast_1d(sources), :] = np.inf
    return x


def test_typed_bf16_under_poison():
    """gnnagg_gat_run_typed: a bf16 x gives bit for bit the fp32 run on x widened, a bf16 y is one rounding of it, newval is unchanged --
    with +Inf, NaN and +0 weights as with ordinary ones"""
    H, D = 8, 16
    F = H * D
    ptr, idx, s, r = logit_graph("bf16")
    V, E = len(ptr) - 1, len(idx)
    gen = torch.Generator().manual_seed(F + H)
    xb = torch.randn((V, F), generator=gen).to(BF)
    x32 = xb.float().numpy()
    att = rand((V, H, 2), 5) * np.float32(0.4)
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    agg.schedule_balanced(16)
    assert agg.balanced_partitions() == 0 and agg.balanced_params() == (16, 16)
    cases = [("clean", att, None), ("wide", wide_att(V, H, 0.2, 7), None)]
    cases += [(what, poisoned(att, where, nodes, h, v), h) for what, where, nodes, h, v in poison_cases("bf16", H, (100.0, float("nan"), -700.0))]
    dxb, dx32 = xb.to(DEV), dev(x32)
    for what, ap, h in cases:
        y32, nv32 = torch.full((V, F), 7.0, device=DEV), torch.full((E, H), 7.0, device=DEV)
        agg.run(dx32, dev(ap), y32, 128, "balanced", heads=H, newval=nv32)
        ref, w = gat_ref_w32(ptr, idx, ap, x32, H)
        zd_el = np.repeat(zero_denominators(ptr, w), D, axis=1)
        y = y32.cpu().numpy()
        assert_same_classes(np.where(zd_el, np.nan, y), ref, "fp32 run, " + what)
        assert plus_zero(y[zd_el]) and plus_zero(y[np.diff(ptr) == 0]), what
        assert_same_classes(nv32.cpu().numpy(), w, "newval, " + what)
        for ydt in (torch.float32, BF):
            yb, nv = torch.full((V, F), 7.0, device=DEV, dtype=ydt), torch.full((E, H), 7.0, device=DEV)
            agg.run(dxb, dev(ap), yb, 128, "balanced", heads=H, newval=nv)
            assert same_t(yb, y32.to(ydt)), "%s, y %s" % (what, ydt)
            assert same_t(nv, nv32), "%s: newval depends on the feature type" % what


@pytest.mark.parametrize("H", [1, 3])
def test_edge_softmax_stages_under_poison(H):
    """gnnagg_gat_run_att computes w_e / sum w unguarded, as attGat: NaN at an Inf edge and +0 at the finite edges of that (row, head),
    NaN on every edge of a zero-denominator (row, head); the three-step baseline (u_add_v, exp on the caller's side, add_to_center,
    div_each) likewise.  On the hub graph of test_gpu_parity.py::test_edge_softmax_kernels_with_hub_rows: hub rows span many items."""
    ptr, idx, s, r = logit_graph("softmax_hubs")
    V, E = len(ptr) - 1, len(idx)
    att = rand((V, H, 2), 4) * np.float32(0.5)
    gat = gnc.Aggregator_GAT(dev(ptr), dev(idx), 32, 32)
    cases = [("clean", None, None, 0, 0.0, att), ("wide", None, None, 0, 0.0, wide_att(V, H, 0.2, 7))]
    cases += [(what, where, nodes, h, v, poisoned(att, where, nodes, h, v))
              for what, where, nodes, h, v in poison_cases("softmax_hubs", H, OVERFLOW + UNDERFLOW)]
    clean_att = None
    for what, where, nodes, h, v, ap in cases:
        out = torch.full((E, H), 7.0, device=DEV)
        gat.run_att(dev(ap), out, 128, heads=H)
        out = out.cpu().numpy()
        with np.errstate(all="ignore"):
            ref = orc.gat_att(ptr, idx, ap, H)
        assert_same_classes(out, ref, "run_att, " + what)
        fin = np.isfinite(ref)
        np.testing.assert_allclose(out[fin], ref[fin], rtol=1e-5, atol=0, err_msg=what)
        if where is not None:
            w = edge_weights32(ptr, idx, ap, H)
            rows = np.repeat(np.arange(V), np.diff(ptr))
            edges_hit = touched_edges(ptr, idx, where, nodes)
            zd_edges = zero_denominators(ptr, w)[rows]
            assert np.isnan(out[zd_edges]).all(), what
            if v in (100.0, float("inf")):
                assert np.isnan(out[edges_hit, h]).all(), what
                rest = touched_rows(ptr, idx, where, nodes)[rows] & ~edges_hit
                assert plus_zero(out[rest, h]), what + ": the finite edges of a (row, head) with an Inf weight"
            mask = np.ones((E, H), bool)
            mask[touched_rows(ptr, idx, where, nodes)[rows], h] = False
            assert np.array_equal(out[mask], clean_att[mask]), what + ": an element outside the head of the rows concerned differs from the clean run"
        elif what == "clean":
            clean_att = out
        if H == 1:
            a2 = ap.reshape(V, 2)
            u = torch.full((E,), 7.0, device=DEV)
            gat.run_u_add_v(dev(a2), u)
            assert same(u.cpu().numpy(), orc.gat_u_add_v(ptr, idx, a2)), what
            wv = torch.exp(torch.nn.functional.leaky_relu(u, 0.2))
            wh = wv.cpu().numpy().copy()
            assert_same_classes(wh, edge_weights32(ptr, idx, ap, 1)[:, 0], "the caller's exp, " + what)
            center = torch.full((V,), 7.0, device=DEV)
            gat.run_add_to_center(wv, center)
            center = center.cpu().numpy()
            with np.errstate(all="ignore"):
                cref = orc.gat_add_to_center(ptr, wh)
            assert_same_classes(center, cref, "add_to_center, " + what)
            fin = np.isfinite(cref)
            np.testing.assert_allclose(center[fin], cref[fin], rtol=1e-5, atol=0, err_msg=what)
            assert plus_zero(center[np.diff(ptr) == 0])
            gat.run_div_each(dev(center), wv)
            assert same(wv.cpu().numpy(), orc.gat_div_each(ptr, center, wh)), "div_each, " + what


@pytest.mark.parametrize("F,H", [(128, 1), (256, 8), (64, 2)])
def test_two_pass_under_poison(F, H):
    """gnnagg_gat_run_part on the split of test_gpu_blocked.py::test_two_pass_gat_on_hub_rows: wide logits, an overflowing source term and
    an underflowing one that leaves no (row, head) without a non-zero weight (a zero denominator is unspecified for this call): the class
    map and the bound of the one-pass balanced run on the union graph; den_io after part 1 holds the first half's denominators."""
    V, E = 3000, 120000
    ptr, idx = hub_graph(V, E, seed=22, alpha=1.0)
    s = poison_sources(ptr, idx, 5)
    assert not captive_rows(ptr, idx, s).any()
    x, att = rand((V, F), 1), rand((V, H, 2), 3) * np.float32(0.4)
    (pa, ia, _), (pb, ib, _) = _split_edges(ptr, idx, None, seed=6)
    a, b, u = (gnc.Aggregator_GAT(dev(p), dev(i), F, F) for p, i in ((pa, ia), (pb, ib), (ptr, idx)))
    h = H // 2
    for what, ap in (("wide", wide_att(V, H, 0.2, 7)), ("overflow", poisoned(att, SRC, s, h, 100.0)), ("underflow", poisoned(att, SRC, s, h, -700.0))):
        y1, y2, den = (torch.full(sh, 7.0, device=DEV) for sh in ((V, F), (V, F), (V, H)))
        u.run(dev(x), dev(ap), y1, 128, "balanced", heads=H)
        a.run_part(dev(x), dev(ap), y2, den, 1, heads=H)
        den = den.cpu().numpy()            # (part 1's denominators; part 2 reads the tensor it is given)
        b.run_part(dev(x), dev(ap), y2, dev(den), 2, heads=H)
        y1, y2 = y1.cpu().numpy(), y2.cpu().numpy()
        ref64, w = gat_ref_w32(ptr, idx, ap, x, H)
        assert not zero_denominators(ptr, w).any()
        assert_same_classes(y1, ref64, "one pass, " + what)
        assert_same_classes(y2, ref64, "two passes, " + what)
        ref = orc.gat_fused(ptr, idx, ap, x, H)
        bound = gat_scale(ptr, idx, ap, x, H) + np.abs(ref)
        fin = np.isfinite(ref64)
        for name, y in (("one pass", y1), ("two passes", y2)):
            ratio = worst_ratio(y, ref, bound, fin)
            assert ratio <= 1, "%s, %s: worst ratio %.3g of the bound" % (name, what, ratio)
        assert plus_zero(y2[np.diff(ptr) == 0])
        # den_io: the first half's denominators, +Inf where one of its edges overflows
        ch, sg = a.balanced_params()
        with np.errstate(all="ignore"):
            da = orc.gat_grouped(*orc.neighbor_grouping(pa, ch), ia, ap, x, V, H, seg=sg)[2]
        assert_same_classes(den, da, "den_io after part 1, " + what)
        fin = np.isfinite(da)
        np.testing.assert_allclose(den[fin], da[fin], rtol=1e-5, atol=0, err_msg=what)
        if what == "overflow":
            assert np.isposinf(den[touched_rows(pa, ia, SRC, s), h]).all() and np.isnan(y2[touched_rows(ptr, idx, SRC, s)][:, head_columns(F, H, h)]).all()
