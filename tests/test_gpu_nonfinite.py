"""GPU: Inf and NaN in the features of every aggregation kernel form.  The kernels pad branch-free -- lanes past a row's end repeat its last
edge with weight 0, lanes past the last feature column accumulate whatever their registers hold, k-quads past K are clamped loads -- and
that is harmless only while 0 . x is 0.  Two inputs make a slip visible:

  Inf columns    x[:, c] = +Inf for EVERY source row, for column 0, column F - 1 and one column inside every head.  A padded lane that
                 multiplies any real source by an exact zero stores a NaN where the value is +-Inf; the other columns must not notice.
  a NaN source   x[s, :] = NaN for one source (a few on a sparse graph, tests/test_nonfinite_host.py::nan_sources; and the last edge's
                 source of the longest row, where the clamps point).  Exactly the rows that have s as a neighbor are NaN, in every column;
                 every other row is bit-equal to the run on the clean x, rows without edges are +0.

The judge is the class map (finite, +Inf, -Inf, NaN) of the float64 numpy references of tests/test_nonfinite_host.py, element for element;
no weight is an exact zero, so the class does not depend on the order of the additions.  Where the suite has a same-order oracle the whole
array is bit-equal to it as well (NaN = NaN).  `max` with a NaN operand is unspecified (include/gnnagg.h) and not tested."""
import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from oracle import oracle as orc
from test_gpu_parity import DEV, assert_within, dev, gat_scale, rand
from test_nonfinite_host import (assert_same_classes, gat_hub_graph, gat_ref64, gcn_ref64, hub_last_source, inf_columns, nan_sources,
                                 poison_inf, poison_nan, powerlaw, reached, signed_weights, weights)

pytestmark = pytest.mark.gpu

_graphs = {}


def graph(name):
    """(ptr, idx, NaN sources, the hub row's last source [with the NaN sources where it alone reaches fewer than 8 rows]), made once"""
    if name not in _graphs:
        ptr, idx = {"powerlaw": lambda: powerlaw(3000, 120000, 5, 1.1),     # short rows, segment rows, hubs (test_gcn_fused_relu)
                    "blocked": lambda: powerlaw(900, 260000, 5, 0.9),        # average degree 289: the 2-D blocked order
                    "nn": lambda: powerlaw(3000, 60000, 5, 1.0),             # test_run_with_nn_fused_epilogue
                    "bf16": lambda: powerlaw(4000, 100000, 9, 1.1),          # tests/test_gpu_bf16.py
                    "forced": lambda: gnc.graph.uniform_random_csr(600, 72000, seed=13),
                    "gat_hubs": gat_hub_graph}[name]()
        s = nan_sources(ptr, idx, 1 if name in ("blocked", "forced") else 5)
        hs = [hub_last_source(ptr, idx)]
        if reached(ptr, idx, hs).sum() < 8:
            hs = hs + s
        _graphs[name] = (ptr, idx, s, hs)
    return _graphs[name]


def nan_rows(ptr, idx, sources):
    """the rows a NaN in `sources` reaches: at least 8 and at most half of all rows"""
    hit = reached(ptr, idx, sources)
    assert 8 <= hit.sum() <= (len(ptr) - 1) // 2, (sources, int(hit.sum()))
    return hit


def same(a, b):
    """bit-for-bit as values, NaN equal to NaN"""
    return np.array_equal(a, b, equal_nan=True)


def plus_zero(a):
    return bool(np.all(a == 0)) and not np.signbit(a).any()


# ------------------------------------------------------------------------------------------------------------------ GCN
GCN_MODES = ["rows", "scheduled32", "scheduled2", "balanced", "blocked", "rows_blocked"]


class Gcn:
    """a handle in one of the kernel forms, the mode argument that reaches it, and the oracle restating the order of its sums"""

    def __init__(self, mode, ptr, idx, val, F):
        self.mode, self.ptr, self.idx, self.val, self.V, self.F = mode, ptr, idx, val, len(ptr) - 1, F
        agg = self.agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), None if val is None else dev(val), F, F)
        self.m = {"rows": 0, "rows_blocked": 0, "scheduled32": 1, "scheduled2": 1, "balanced": "balanced", "blocked": "balanced"}[mode]
        if mode == "rows":
            agg.set_option("fast_rows", 0)                         # the canonical CSR-order chains
            agg.set_option("rows_blocked", 0)
        elif mode in ("scheduled32", "scheduled2"):                # the user's groups in the restated order: the plan kernel (NG = 32),
            self.ng = int(mode[9:])                                # the item kernels + k_combine (NG = 2)
            agg.set_option("fast_scheduled", 0)
            agg.schedule(gnc.Schedule.neighbor_grouping, [self.ng])
        elif mode == "balanced":
            agg.schedule_balanced(16)                              # short rows, segment rows, the in-kernel hub fold
            chunk, seg = agg.balanced_params()
            assert int(np.diff(ptr).max()) > 2 * chunk * seg
        elif mode == "blocked":
            agg.set_option("slice_kb", 16)
            assert agg.balanced_partitions() > 1
        elif mode == "rows_blocked":
            agg.set_option("slice_kb", 16)
            assert agg.rows_blocked_ranges() > 1

    def run(self, x, **kw):
        y = torch.full((self.V, self.F), 7.0, device=DEV)
        self.agg.run(dev(x), y, 128, self.m, **kw)
        return y

    def same_order_sum(self, x):
        ptr, idx, val, V, agg = self.ptr, self.idx, self.val, self.V, self.agg
        if self.mode in ("rows", "rows_blocked"):
            return orc.gcn_seq(ptr, idx, val, x)
        if self.mode in ("scheduled32", "scheduled2"):
            ps, tg = orc.neighbor_grouping(ptr, self.ng)
            return orc.gcn_grouped(ps, tg, idx, val, x, V, seg=agg.mode_params("scheduled")[1])
        if self.mode == "balanced":
            ps, _, tg = agg.get_schedule("balanced")
            return orc.gcn_grouped(ps, tg, idx, val, x, V, seg=agg.balanced_params()[1])
        chunk, seg = agg.balanced_params()
        assert seg == 0
        ps, ix, tg, vs = orc.locality_schedule(ptr, idx, agg.balanced_partitions(), agg.balanced_partition_columns(), ng=chunk, val=val)
        return orc.gcn_grouped(ps, tg, ix, vs, x, V, seg=0)


def gcn_case(mode, F, val_kind):
    ptr, idx, s, hs = graph("blocked" if mode in ("blocked", "rows_blocked") else "powerlaw")
    val = {"none": lambda: None, "positive": lambda: weights(len(idx), 2, positive=True), "signed": lambda: signed_weights(ptr, 2)}[val_kind]()
    return Gcn(mode, ptr, idx, val, F), ptr, idx, val, rand((len(ptr) - 1, F), 1), s, hs


@pytest.mark.parametrize("F", [128, 100, 33, 602])
@pytest.mark.parametrize("mode", GCN_MODES)
def test_gcn_inf_columns(mode, F):
    cols = inf_columns(F)
    other = np.setdiff1d(np.arange(F), cols)
    for val_kind in ("signed", "positive", "none"):
        g, ptr, idx, val, x, _, _ = gcn_case(mode, F, val_kind)
        deg = np.diff(ptr)
        xi = poison_inf(x, cols)
        ref = gcn_ref64(ptr, idx, val, xi)
        for red in ("sum", "mean"):
            what = "%s F=%d val=%s %s" % (mode, F, val_kind, red)
            y, y_clean = g.run(xi, reduce=red).cpu().numpy(), g.run(x, reduce=red).cpu().numpy()
            assert_same_classes(y, ref, what)                                  # (a mean is the sum over a positive finite count)
            assert np.array_equal(y[:, other], y_clean[:, other]), what + ": a column without an Inf differs from the clean run"
            assert np.isfinite(y_clean).all()
            if val_kind != "signed":                                           # weights of one sign: +Inf, a NaN is not allowed
                assert np.isposinf(y[deg > 0][:, cols]).all() and not np.isnan(y).any(), what
            assert plus_zero(y[deg == 0]), what
            if red == "sum":
                assert same(y, g.same_order_sum(xi)), what + ": not the oracle's sums in the order the run used"
            elif g.m == 0:
                assert same(y, orc.gcn_mean(ptr, idx, val, xi)), what
        if val_kind == "positive":
            continue
        y, y_clean = g.run(xi, reduce="max").cpu().numpy(), g.run(x, reduce="max").cpu().numpy()
        what = "%s F=%d val=%s max" % (mode, F, val_kind)
        assert_same_classes(y, gcn_ref64(ptr, idx, val, xi, "max"), what)
        assert np.array_equal(y[:, other], y_clean[:, other]) and same(y, orc.gcn_max(ptr, idx, val, xi)), what
        if val_kind == "signed":
            # the fused ReLU is clamp_min of the unfused run (test_gcn_fused_relu): NaN stays NaN, -Inf becomes 0
            for red in ("sum", "mean"):
                y_plain = g.run(xi, reduce=red)
                expect = torch.clamp_min(y_plain, 0.0).cpu().numpy()
                assert np.isnan(expect).any() and np.isposinf(expect).any() and np.isneginf(y_plain.cpu().numpy()).any() and not np.isneginf(expect).any()
                assert same(g.run(xi, reduce=red, relu=True).cpu().numpy(), expect), "%s F=%d %s + ReLU" % (mode, F, red)
            if mode == "balanced":
                base = rand((len(ptr) - 1, F), 3)
                ya, yc = dev(base).clone(), dev(base).clone()
                g.agg.run(dev(xi), ya, 128, "balanced", accumulate=True)
                g.agg.run(dev(x), yc, 128, "balanced", accumulate=True)
                assert_same_classes(ya.cpu().numpy(), ref + base, "accumulate")
                assert torch.equal(ya[:, other], yc[:, other])
                assert same(ya.cpu().numpy(), (dev(base) + g.run(xi)).cpu().numpy())


@pytest.mark.parametrize("F", [128, 100, 33, 602])
@pytest.mark.parametrize("mode", GCN_MODES)
def test_gcn_one_nan_source(mode, F):
    for val_kind in ("signed", "none"):
        g, ptr, idx, val, x, s, hs = gcn_case(mode, F, val_kind)
        deg = np.diff(ptr)
        for sources in (s, hs):
            hit = nan_rows(ptr, idx, sources)
            xn = poison_nan(x, sources)
            ref = gcn_ref64(ptr, idx, val, xn)
            assert np.array_equal(np.isnan(ref).all(axis=1), hit) and np.array_equal(np.isnan(ref).any(axis=1), hit)
            for red in ("sum", "mean"):
                what = "%s F=%d val=%s %s, NaN in x[%s]" % (mode, F, val_kind, red, sources)
                y, y_clean = g.run(xn, reduce=red).cpu().numpy(), g.run(x, reduce=red).cpu().numpy()
                assert_same_classes(y, ref, what)
                assert np.isnan(y[hit]).all(), what
                assert np.array_equal(y[~hit], y_clean[~hit]), what + ": a row that does not have the source as a neighbor differs from the clean run"
                assert plus_zero(y[deg == 0]), what
                if red == "sum":
                    assert same(y, g.same_order_sum(xn)), what
                elif g.m == 0:
                    assert same(y, orc.gcn_mean(ptr, idx, val, xn)), what
                y_plain = g.run(xn, reduce=red)
                expect = torch.clamp_min(y_plain, 0.0).cpu().numpy()          # NaN stays NaN
                assert np.array_equal(np.isnan(expect).all(axis=1), hit)
                assert same(g.run(xn, reduce=red, relu=True).cpu().numpy(), expect), what + " + ReLU"
        if mode == "balanced" and val_kind == "signed":
            xn = poison_nan(x, s)
            base = rand((len(ptr) - 1, F), 3)
            for relu in (False, True):
                ya, yc = dev(base).clone(), dev(base).clone()
                g.agg.run(dev(xn), ya, 128, "balanced", accumulate=True, relu=relu)
                g.agg.run(dev(x), yc, 128, "balanced", accumulate=True, relu=relu)
                hit = reached(ptr, idx, s)
                assert bool(torch.isnan(ya[dev(hit)]).all()) and torch.equal(ya[dev(~hit)], yc[dev(~hit)]), "accumulate, relu=%s" % relu


@pytest.mark.parametrize("mode", ["rows", "balanced"])
@pytest.mark.parametrize("F,OUT", [(128, 32), (100, 7), (30, 33), (602, 32)])
def test_run_with_nn_fused_epilogue(mode, F, OUT):
    """y as above; t = y . W by the class map of the float64 product of the float64 y, and bit-equal to the oracle's GEMM of the y the run wrote"""
    ptr, idx, s, hs = graph("nn")
    V, E = len(ptr) - 1, len(idx)
    x, val, w = rand((V, F), 1), weights(E, 2), weights((F, OUT), 3)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, OUT)
    m = {"rows": 0, "balanced": "balanced"}[mode]
    dw = dev(w)

    def order(xp):
        if mode == "rows":
            return orc.gcn_seq(ptr, idx, val, xp)
        ps, _, tg = agg.get_schedule("balanced")
        return orc.gcn_grouped(ps, tg, idx, val, xp, V, seg=agg.balanced_params()[1])

    def run(xp):
        y, t = torch.full((V, F), 7.0, device=DEV), torch.full((V, OUT), 7.0, device=DEV)
        agg.run_with_nn(dev(xp), y, dw, t, 128, m)
        y_plain = torch.full((V, F), 7.0, device=DEV)
        agg.run(dev(xp), y_plain, 128, m)
        assert same(y.cpu().numpy(), y_plain.cpu().numpy())
        return y.cpu().numpy(), t.cpu().numpy()

    y_clean, t_clean = run(x)
    assert np.array_equal(y_clean, order(x)) and np.array_equal(t_clean, orc.matmul_nn(y_clean, w))
    cols = inf_columns(F)
    for what, xp in (("Inf columns", poison_inf(x, cols)), ("NaN source", poison_nan(x, s)), ("NaN in the hub's last source", poison_nan(x, hs))):
        y, t = run(xp)
        ref = gcn_ref64(ptr, idx, val, xp)
        assert_same_classes(y, ref, "y, " + what)
        assert same(y, order(xp)), what
        with np.errstate(invalid="ignore"):
            t_ref = ref @ w.astype(np.float64)
        assert_same_classes(t, t_ref, "t, " + what)
        assert same(t, orc.matmul_nn(y, w)), what
        if what == "Inf columns":
            other = np.setdiff1d(np.arange(F), cols)
            assert np.array_equal(y[:, other], y_clean[:, other])
            assert not np.isfinite(t[np.diff(ptr) > 0]).any()       # a non-zero W: every product of a row with edges meets an Inf
        else:
            hit = nan_rows(ptr, idx, s if what == "NaN source" else hs)
            assert np.isnan(y[hit]).all() and np.isnan(t[hit]).all()
            assert np.array_equal(y[~hit], y_clean[~hit]) and np.array_equal(t[~hit], t_clean[~hit])


# ------------------------------------------------------------------------------------------------------------------ GAT
def gat_handle(mode, ptr, idx, F, opts):
    gat = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    if mode == "rows":
        return gat, 0
    if mode == "scheduled":
        gat.set_option("fast_scheduled", 0)
        gat.schedule(gnc.Schedule.neighbor_grouping, [32])
        return gat, 1
    if mode == "balanced":
        gat.schedule_balanced(16)
        return gat, "balanced"
    gat.set_option("slice_kb", 16)
    for k, v in opts.items():
        gat.set_option(k, v)
    assert gat.balanced_partitions() > 1
    return gat, "balanced"


GAT_CASES = ([("blocked", F, H, {}) for F, H in ((256, 8), (64, 1), (96, 3), (30, 3))] +
             # k_gat_span's other lane-group widths (test_blocked_gat_span_kernel_variants): partial last windows of every GROUP
             [("blocked", 128, 4, {"tile_width": 32}), ("blocked", 64, 1, {"tile_width": 32}), ("blocked", 256, 8, {"tile_width": 128})] +
             [(mode, F, H, {}) for mode in ("rows", "scheduled", "balanced") for F, H in ((128, 1), (256, 8))])


@pytest.mark.parametrize("mode,F,H,opts", GAT_CASES, ids=lambda v: "-".join("%s%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_gat_inf_columns_and_one_nan_source(mode, F, H, opts):
    ptr, idx, s, hs = graph({"blocked": "blocked", "balanced": "gat_hubs"}.get(mode, "powerlaw"))
    V, E = len(ptr) - 1, len(idx)
    deg = np.diff(ptr)
    x, att = rand((V, F), 1), rand((V, H, 2), 2) * np.float32(0.4)
    gat, m = gat_handle(mode, ptr, idx, F, opts)
    datt = dev(att)

    def run(xp, with_newval):
        y = torch.full((V, F), 7.0, device=DEV)
        nv = torch.full((E, H), 7.0, device=DEV) if with_newval else None
        gat.run(dev(xp), datt, y, 128, m, heads=H, newval=nv)
        return y.cpu().numpy(), nv

    cols = inf_columns(F, H)
    other = np.setdiff1d(np.arange(F), cols)
    ref = orc.gat_fused(ptr, idx, att, x, H)
    bound = gat_scale(ptr, idx, att, x, H) + np.abs(ref)
    ref_inf = gat_ref64(ptr, idx, att, poison_inf(x, cols), H)
    ref_nan = {tuple(src): gat_ref64(ptr, idx, att, poison_nan(x, src), H) for src in (s, hs)}
    for with_newval in (True, False):
        y_clean, nv_clean = run(x, with_newval)
        # the finite elements stay within the suite's bound: they are the clean run's, and the clean run meets the bound
        assert_within(y_clean, ref, bound, "gat %s, clean x" % mode)
        y, nv = run(poison_inf(x, cols), with_newval)
        what = "gat %s F=%d H=%d %s newval=%s, Inf columns" % (mode, F, H, opts, with_newval)
        assert_same_classes(y, ref_inf, what)
        assert np.isposinf(y[deg > 0][:, cols]).all() and not np.isnan(y).any(), what     # positive weights: +Inf, never NaN
        assert plus_zero(y[deg == 0]), what
        assert np.array_equal(y[:, other], y_clean[:, other]), what + ": a column without an Inf differs from the clean run"
        assert nv is None or torch.equal(nv, nv_clean), what + ": newval depends on x"
        for sources in (s, hs):
            hit = nan_rows(ptr, idx, sources)
            xn = poison_nan(x, sources)
            y, nv = run(xn, with_newval)
            what = "gat %s F=%d H=%d %s newval=%s, NaN in x[%s]" % (mode, F, H, opts, with_newval, sources)
            assert_same_classes(y, ref_nan[tuple(sources)], what)
            assert np.isnan(y[hit]).all(), what
            assert np.array_equal(y[~hit], y_clean[~hit]), what + ": a row that does not have the source as a neighbor differs from the clean run"
            assert plus_zero(y[deg == 0]), what
            assert nv is None or torch.equal(nv, nv_clean), what + ": newval depends on x"


# ------------------------------------------------------------------------------------------------------------------ bf16
BF = torch.bfloat16


def same_t(a, b):
    """torch.equal with NaN positions compared by isnan"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def bf16_patterns(name, F, H=1):
    """[(what, bf16-representable poisoned x as fp32 numpy, rows a NaN reaches or None)] and the clean x"""
    ptr, idx, s, hs = graph(name)
    V = len(ptr) - 1
    g = torch.Generator().manual_seed(F + H)
    x = torch.randn((V, F), generator=g).to(BF).float().numpy()
    return x, [("Inf columns", poison_inf(x, inf_columns(F, H)), None), ("NaN source", poison_nan(x, s), nan_rows(ptr, idx, s)),
               ("NaN in the hub's last source", poison_nan(x, hs), nan_rows(ptr, idx, hs))]


@pytest.mark.parametrize("case", ["balanced_powerlaw", "forced_partitions"])
def test_gcn_typed_bf16(case):
    name, F = ("bf16", 128) if case == "balanced_powerlaw" else ("forced", 100)
    ptr, idx, _, _ = graph(name)
    V, E = len(ptr) - 1, len(idx)
    val = weights(E, 4)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)
    f32 = agg
    if case == "balanced_powerlaw":
        agg.schedule_balanced(16)
    else:
        agg.set_option("partitions", 16)               # 16-bit features run the chunked plan: the fp32 run of that order is a handle
        f32 = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)    # without source partitions
        f32.set_option("partitions", 0)
        assert agg.balanced_partitions() == 16 and f32.balanced_partitions() == 0
    x, patterns = bf16_patterns(name, F)
    for what, xp, hit in patterns:
        y32 = torch.full((V, F), 7.0, device=DEV)
        f32.run(dev(xp), y32, 512, "balanced")
        assert_same_classes(y32.cpu().numpy(), gcn_ref64(ptr, idx, val, xp), "%s, fp32 run, %s" % (case, what))
        assert hit is None or np.array_equal(np.isnan(y32.cpu().numpy()).all(axis=1), hit)
        for ydt in (torch.float32, BF):
            yb = torch.full((V, F), 7.0, device=DEV, dtype=ydt)
            agg.run(dev(xp).to(BF), yb, 512, "balanced")
            assert same_t(yb, y32.to(ydt)), "%s, %s, y %s" % (case, what, ydt)


@pytest.mark.parametrize("case", ["balanced_powerlaw", "forced_partitions"])
def test_gat_typed_bf16(case):
    name, H, D = ("bf16", 8, 16) if case == "balanced_powerlaw" else ("forced", 8, 16)
    F = H * D
    ptr, idx, _, _ = graph(name)
    V, E = len(ptr) - 1, len(idx)
    att = rand((V, H, 2), 5) * np.float32(0.4)
    datt = dev(att)
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    f32 = agg
    if case == "balanced_powerlaw":
        agg.schedule_balanced(16)
    else:
        agg.set_option("partitions", 16)
        f32 = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
        f32.set_option("partitions", 0)
        assert agg.balanced_partitions() == 16 and f32.balanced_partitions() == 0
    x, patterns = bf16_patterns(name, F, H)
    nv_clean = torch.full((E, H), 7.0, device=DEV)
    f32.run(dev(x), datt, torch.empty((V, F), device=DEV), 128, "balanced", heads=H, newval=nv_clean)
    for what, xp, hit in patterns:
        y32 = torch.full((V, F), 7.0, device=DEV)
        f32.run(dev(xp), datt, y32, 128, "balanced", heads=H)
        assert_same_classes(y32.cpu().numpy(), gat_ref64(ptr, idx, att, xp, H), "%s, fp32 run, %s" % (case, what))
        assert hit is None or np.array_equal(np.isnan(y32.cpu().numpy()).all(axis=1), hit)
        for ydt in (torch.float32, BF):
            yb, nv = torch.full((V, F), 7.0, device=DEV, dtype=ydt), torch.full((E, H), 7.0, device=DEV)
            agg.run(dev(xp).to(BF), datt, yb, 128, "balanced", heads=H, newval=nv)
            assert same_t(yb, y32.to(ydt)), "%s, %s, y %s" % (case, what, ydt)
            assert torch.equal(nv, nv_clean), "newval depends on x"
