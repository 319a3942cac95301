"""CPU: the generators and judges of tests/test_gpu_multi_aggr_nonfinite.py, each checked on the host.

The contract (include/gnnagg.h, "non-finite" under gnnagg_gcn_run_multi): sum, mean, var and std have the class map (finite / +Inf / -Inf /
NaN, element for element) of multi_ref, the float64 two-moment reference over the fp32 messages -- var and std are NaN wherever a message
of the (row, column) is +-Inf or NaN; min and max SKIP NaN messages (np.fmin / np.fmax), are exact on +-Inf, and are NaN where every
message of the (row, column) is NaN; every (row, column) that no non-finite message reaches keeps the bits of the run without it.

* multi_ref_nf: multi_ref with min / max by np.fmin / np.fmax;
* nf_x / nf_val: the fixture's features and edge values with their exact zeros redrawn (Inf * 0 would be a NaN of the reference's own);
* poison_val: edge-exact poisoning (val[p] = +Inf, -Inf, NaN or 0 at chosen edges);
* idx_reserved: source-exact poisoning (one source id named by exactly a given edge list);
* long_positions / short_positions / position_runs: where inside a row the poisoned edge stands (batch, window, chunk, segment, slot);
* locate: the (segment, lane group) of an edge of a long row, restated from k_multi_aggr;
* reach_map: the (row, column) pairs a non-finite message reaches;
* the themes: the inputs of every GPU theme, so that the host can run the float32 restatement over the same inputs.
"""
import functools

import numpy as np
import pytest

from test_multi_aggr_host import (AGGRS, BATCH, DEGREES, LONG_EDGES, SEG_EDGES, fixture_graph, fixture_val, fixture_x, messages32,
                                  multi_chain32, multi_geometry, multi_ref, tiny_graph)
from test_nonfinite_host import FINITE, NAN, NINF, PINF, assert_same_classes, classes
from test_nonfinite_host import nonzero as redraw_zeros

INF = np.float32(np.inf)
QNAN = np.float32(np.nan)
GPB = {8: 8, 16: 8, 32: 8, 64: 4}            # lane groups per workgroup (block_of<GROUP>() / GROUP, csrc/kernel_util.cuh)
NF_F = (5, 128, 602, 1024)                   # scalar and packed lanes at 1, 10 and 4 fragments
SRC_PINF, SRC_NINF, SRC_NAN = 3, 17, 11      # the three poisoned sources of theme 1
RESERVED = 20                                # the source of idx_reserved (RESERVED + 1 takes its edges)


# ------------------------------------------------------------------------------------------------ reference
def multi_ref_nf(ptr, idx, val, x):
    """multi_ref with the contract's min / max: NaN messages skipped (np.fmin / np.fmax over the fp32 messages), NaN where all are NaN"""
    out = dict(multi_ref(ptr, idx, val, x))
    with np.errstate(invalid="ignore", over="ignore"):
        m = messages32(idx, val, x)
    out["min"], out["max"] = np.zeros_like(out["min"]), np.zeros_like(out["max"])
    for r in range(len(ptr) - 1):
        b, e = int(ptr[r]), int(ptr[r + 1])
        if e > b:
            out["min"][r] = np.fmin.reduce(m[b:e], axis=0)
            out["max"][r] = np.fmax.reduce(m[b:e], axis=0)
    return out


def reach_map(ptr, idx, val, x):
    """bool [V, F]: (row, column) pairs with a non-finite message"""
    with np.errstate(invalid="ignore", over="ignore"):
        bad = ~np.isfinite(messages32(idx, val, x))
    out = np.zeros((len(ptr) - 1, x.shape[1]), bool)
    for r in range(len(ptr) - 1):
        b, e = int(ptr[r]), int(ptr[r + 1])
        if e > b:
            out[r] = bad[b:e].any(0)
    return out


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def nf_x(F):
    x = redraw_zeros(fixture_x(F))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def nf_val():
    v = redraw_zeros(fixture_val())
    v.setflags(write=False)
    return v


def poison_val(val, edges, value):
    v = np.array(val, np.float32, copy=True)
    v[np.asarray(edges, np.int64)] = np.float32(value)
    return v


def idx_reserved(idx, u, edges):
    """idx in which source u is named by exactly `edges` (its other edges move to u + 1: the trick of
    test_a_source_row_that_no_edge_names_is_never_read_into_a_result)"""
    out = idx.copy()
    out[out == u] = u + 1
    out[np.asarray(edges, np.int64)] = u
    return out


# ------------------------------------------------------------------------------------------------ positions
def chunk_edges(seg_len, gpb):
    """k_multi_aggr: the edges of a lane group's chunk of a segment -- ceil(len / GPB) rounded up to the batch"""
    c = -(-seg_len // gpb)
    return -(-c // BATCH) * BATCH


def locate(deg, pos, gpb):
    """(segment, lane group, lane groups of the segment that have edges) of edge `pos` of a row of deg > LONG_EDGES edges"""
    assert deg > LONG_EDGES and 0 <= pos < deg
    s = pos // SEG_EDGES
    seg_len = min(SEG_EDGES, deg - s * SEG_EDGES)
    c = chunk_edges(seg_len, gpb)
    return s, (pos - s * SEG_EDGES) // c, -(-seg_len // c)


def long_positions(deg, gpb):
    """edge 0, the last edge of the first batch, the first edge of the second lane group's chunk, edges 511 and 512 (either side of the
    first segment boundary), one edge past 1024 (the third segment), edge 1099 and the row's last edge -- those the row has"""
    cand = [0, BATCH - 1, chunk_edges(min(deg, SEG_EDGES), gpb), SEG_EDGES - 1, SEG_EDGES, 2 * SEG_EDGES + 1, 1099, deg - 1]
    return sorted({p for p in cand if 0 <= p < deg})


def short_positions(deg, group):
    return sorted({p for p in (0, deg - 1, group - 1, group) if 0 <= p < deg})


def row_positions(deg, group):
    return short_positions(deg, group) if deg <= LONG_EDGES else long_positions(deg, GPB[group])


def position_runs(ptr, group):
    """one list of global edge positions per run: run k holds the k-th position of every row that has one (rows are independent, so one
    position per row per run)"""
    per_row = [row_positions(int(d), group) for d in np.diff(ptr)]
    n = max(len(p) for p in per_row)
    return [[int(ptr[r]) + p[k] for r, p in enumerate(per_row) if k < len(p)] for k in range(n)]


def group_of(F, esize=4):
    return multi_geometry(F, esize)[1]


# ------------------------------------------------------------------------------------------------ themes
PTR, IDX, N_SRC = fixture_graph()
V = len(PTR) - 1
DEG = np.diff(PTR)
ROW_1100 = DEGREES.index(1100)


def case(label, x, val=None, idx=None, clean_x=None, clean_val=None):
    """one GPU run and the run without the poison it is compared with"""
    return dict(label=label, idx=IDX if idx is None else idx, x=x, val=val, clean_x=x if clean_x is None else clean_x,
                clean_val=val if clean_val is None else clean_val)


def theme_sources(F, with_val):
    """theme 1: +Inf, -Inf and NaN in three sources, on all columns and on one"""
    x0, val = nf_x(F), (nf_val() if with_val else None)
    out = []
    for what, cols in (("all columns", slice(None)), ("column %d" % (F // 2), F // 2)):
        x = x0.copy()
        x[SRC_PINF, cols], x[SRC_NINF, cols], x[SRC_NAN, cols] = INF, -INF, QNAN
        out.append(case("sources %d / %d / %d = +Inf / -Inf / NaN on %s" % (SRC_PINF, SRC_NINF, SRC_NAN, what), x, val, clean_x=x0))
    return out


def theme_positions(F, value):
    """theme 2: val[p] = value at one position per row per run"""
    x, val = nf_x(F), nf_val()
    return [case("val = %s at run %d of the position list" % (value, k), x, poison_val(val, edges, value), clean_val=val)
            for k, edges in enumerate(position_runs(PTR, group_of(F)))]


def theme_all_nan(F):
    """theme 3: a column of x entirely NaN (without and with val); through val, the middle segment of the 1100-edge row entirely NaN"""
    x0, val = nf_x(F), nf_val()
    col = F // 3
    x = x0.copy()
    x[:, col] = QNAN
    b = int(PTR[ROW_1100])
    seg = np.arange(b + SEG_EDGES, b + 2 * SEG_EDGES)
    return [case("column %d of x all NaN, no val" % col, x, None, clean_x=x0), case("column %d of x all NaN, val" % col, x, val, clean_x=x0),
            case("val = NaN over the second segment of the 1100-edge row", x0, poison_val(val, seg, QNAN), clean_val=val)]


def theme_zero_times_inf(F):
    """theme 4: source RESERVED holds +Inf and is named by the edges of three runs of the position list; val = 0 on two of them (a NaN
    message, formed by the walk), the edges of the third keep their signed value (an Inf message)"""
    runs = position_runs(PTR, group_of(F))
    zero = sorted(set(runs[0]) | set(runs[2]))
    named = sorted(set(zero) | set(runs[1]))
    idx = idx_reserved(IDX, RESERVED, named)
    x0, val = nf_x(F), nf_val()
    x = x0.copy()
    x[RESERVED] = INF
    v = poison_val(val, zero, 0.0)
    return [case("val = 0 on edges whose source holds +Inf", x, v, idx, clean_x=x0, clean_val=v)]


def all_themes(F):
    out = theme_sources(F, False) + theme_sources(F, True) + theme_all_nan(F) + theme_zero_times_inf(F)
    for value in (QNAN, INF):
        out += theme_positions(F, value)
    return out


# ------------------------------------------------------------------------------------------------ tests
def brute(ms):
    """the six aggregates of a list of fp32 messages by the rules of the contract, in plain Python"""
    d = len(ms)
    f = [float(m) for m in ms]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.float64(0)
        q = np.float64(0)
        for v in f:
            s = s + np.float64(v)
            q = q + np.float64(v) * np.float64(v)
        mean = s / d
        var = q / d - mean * mean
        var = var if np.isnan(var) else max(var, 0.0)
        kept = [v for v in f if v == v]
        mn = min(kept) if kept else float("nan")
        mx = max(kept) if kept else float("nan")
    return {"sum": s, "mean": mean, "min": mn, "max": mx, "var": var, "std": np.sqrt(var)}


@pytest.mark.parametrize("with_val", [False, True])
def test_multi_ref_nf_against_a_brute_force_loop(with_val):
    ptr, idx, x, val = tiny_graph()
    x = x.copy()
    x[0, 0] = INF              # column 0: one +Inf (rows 2 and 4 gather source 0 / not)
    x[1, 1] = QNAN             # column 1: a NaN beside finite messages
    x[:, 2] = QNAN             # column 2: all NaN
    x2 = x.copy()
    x2[3, 0] = -INF            # column 0 of row 2: both infinities (sources 0, 0, 3)
    val = val if with_val else None
    for xs in (x, x2):
        ref = multi_ref_nf(ptr, idx, val, xs)
        for r in range(5):
            for c in range(3):
                ms = [np.float32(xs[idx[p], c]) if val is None else np.float32(np.float32(val[p]) * np.float32(xs[idx[p], c]))
                      for p in range(ptr[r], ptr[r + 1])]
                if not ms:
                    assert all(ref[k][r, c] == 0 for k in AGGRS)
                    continue
                want = brute(ms)
                for k in AGGRS:
                    g, w = ref[k][r, c], want[k]
                    assert classes(g) == classes(w), (r, c, k, g, w)
                    if np.isfinite(w):
                        assert g == pytest.approx(w, rel=1e-9, abs=1e-12), (r, c, k)
        assert np.isnan(ref["min"][:, 2][[1, 2, 4]]).all() and np.isnan(ref["max"][:, 2][[1, 2, 4]]).all()      # all-NaN: NaN, never a seed
        assert np.isnan(ref["var"][2, 0]) and np.isnan(ref["std"][2, 0]) and np.isnan(ref["var"][4, 1])
    if val is None:
        assert ref["min"][2, 0] == -np.inf and ref["max"][2, 0] == np.inf and np.isnan(ref["sum"][2, 0])            # both infinities
    assert np.isfinite(ref["min"][4, 1]) and np.isfinite(ref["max"][4, 1])                                          # the NaN was skipped


@pytest.mark.parametrize("with_val", [False, True])
def test_multi_ref_nf_is_multi_ref_on_finite_input(with_val):
    val = nf_val() if with_val else None
    a, b = multi_ref(PTR, IDX, val, nf_x(5)), multi_ref_nf(PTR, IDX, val, nf_x(5))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not reach_map(PTR, IDX, val, nf_x(5)).any()


def test_generators_leave_no_exact_zero_and_poison_exactly():
    for F in NF_F:
        assert not (nf_x(F) == 0).any() and nf_x(F).dtype == np.float32
    val = nf_val()
    assert not (val == 0).any() and (val > 0).any() and (val < 0).any()
    v = poison_val(val, [0, 5], -INF)
    assert np.array_equal(np.flatnonzero(v != val), [0, 5]) and (v[[0, 5]] == -np.inf).all()
    edges = [int(PTR[5]), int(PTR[ROW_1100]) + 600]
    idx = idx_reserved(IDX, RESERVED, edges)
    assert np.array_equal(np.flatnonzero(idx == RESERVED), sorted(edges)) and (IDX == RESERVED).sum() > 2
    moved = (IDX == RESERVED) & (idx != RESERVED)
    assert (idx[moved] == RESERVED + 1).all() and idx.max() < N_SRC
    same = ~moved
    same[edges] = False
    assert np.array_equal(idx[same], IDX[same])
    assert len({SRC_PINF, SRC_NINF, SRC_NAN, RESERVED, RESERVED + 1}) == 5 and max(SRC_NINF, RESERVED + 1) < N_SRC


def test_position_lists_name_the_edges_of_the_walk():
    assert [group_of(F) for F in NF_F] == [8, 32, 64, 64] and group_of(13) == 16
    assert long_positions(1100, 8) == [0, 3, 64, 511, 512, 1025, 1099] and long_positions(1100, 4) == [0, 3, 128, 511, 512, 1025, 1099]
    assert long_positions(129, 8) == [0, 3, 20, 128] and long_positions(513, 4) == [0, 3, 128, 511, 512]
    assert long_positions(512, 8) == [0, 3, 64, 511] and long_positions(130, 4) == [0, 3, 36, 129]
    for g in (8, 16, 32, 64):
        assert short_positions(g + 1, g) == [0, g - 1, g] and short_positions(g, g) == [0, g - 1] and short_positions(1, g) == [0]
        runs = position_runs(PTR, g)
        flat = [p for run in runs for p in run]
        assert len(set(flat)) == len(flat) and len(runs) == 7
        rows = [np.searchsorted(PTR, run, side="right") - 1 for run in runs]
        for run, rs in zip(runs, rows):
            assert len(set(rs)) == len(rs), "two poisoned edges in one row of one run"
            assert all(PTR[r] <= p < PTR[r + 1] for p, r in zip(run, rs))
        assert set(rows[0]) == set(np.flatnonzero(DEG > 0))            # run 0: edge 0 of every row that has edges
        per_row = {r: sorted(p - int(PTR[r]) for run in runs for p in run if PTR[r] <= p < PTR[r + 1]) for r in range(V)}
        for r in range(V):
            assert per_row[r] == row_positions(int(DEG[r]), g)


@pytest.mark.parametrize("gpb", [8, 4])
def test_positions_hit_every_chunk_and_slot_class_of_the_1100_edge_row(gpb):
    """the first chunk of a segment, the last chunk of a segment, the 76-edge third segment (whose chunks are 12 edges at 8 lane groups
    per workgroup -- the eighth is empty, the seventh holds 4 -- and 20 at 4), and a slot that holds only poisoned edges"""
    where = {p: locate(1100, p, gpb) for p in long_positions(1100, gpb)}
    assert where[0][:2] == (0, 0) and where[SEG_EDGES][:2] == (1, 0)                              # first chunk of a segment
    assert where[SEG_EDGES - 1] == (0, gpb - 1, gpb)                                              # last chunk of a full segment
    assert where[1099][0] == 2 and where[1099][1] == where[1099][2] - 1                           # last chunk that has edges, third segment
    assert where[2 * SEG_EDGES + 1][:2] == (2, 0)
    assert where[chunk_edges(SEG_EDGES, gpb)][:2] == (0, 1) and where[BATCH - 1][:2] == (0, 0)    # second lane group's first edge
    assert chunk_edges(76, 8) == 12 and locate(1100, 1099, 8) == (2, 6, 7) and chunk_edges(76, 4) == 20 and locate(1100, 1099, 4) == (2, 3, 4)
    # the all-NaN theme's val case: exactly the edges of the row's second segment, i.e. of its second scratch slot
    c = theme_all_nan(5)[2]
    bad = np.flatnonzero(np.isnan(c["val"])) - int(PTR[ROW_1100])
    assert np.array_equal(bad, np.arange(SEG_EDGES, 2 * SEG_EDGES)) and {locate(1100, int(p), gpb)[0] for p in bad} == {1}
    assert np.isfinite(c["clean_val"]).all()


def test_restatement_has_the_reference_classes_on_every_theme():
    """multi_chain32 (the kernel's float32 chains on short rows) and multi_ref_nf give the same class map for sum, mean, var and std on
    every input the GPU file runs: the GPU judge is then the reference alone"""
    F = 5
    n = 0
    for c in all_themes(F):
        ref, c32 = multi_ref_nf(PTR, c["idx"], c["val"], c["x"]), multi_chain32(PTR, c["idx"], c["val"], c["x"])
        for k in ("sum", "mean", "var", "std"):
            assert_same_classes(c32[k], ref[k], "%s, %s" % (c["label"], k))
        reach = reach_map(PTR, c["idx"], c["val"], c["x"])
        assert reach.any() and not reach[DEG == 0].any()
        assert np.isnan(ref["var"][reach]).all() and np.isnan(ref["std"][reach]).all(), c["label"]
        assert np.isfinite(ref["var"][~reach]).all()
        clean = multi_chain32(PTR, c["idx"], c["clean_val"], c["clean_x"])
        for k in ("sum", "mean", "var", "std"):
            assert np.array_equal(c32[k][~reach], clean[k][~reach]), "%s: %s changed where nothing non-finite reaches" % (c["label"], k)
        assert not reach_map(PTR, c["idx"], c["clean_val"], c["clean_x"]).any()
        n += 1
    assert n == 2 + 2 + 3 + 1 + 2 * 7


def test_themes_show_every_class_the_contract_names():
    F = 5
    seen = {k: set() for k in AGGRS}
    for c in all_themes(F):
        ref = multi_ref_nf(PTR, c["idx"], c["val"], c["x"])
        for k in AGGRS:
            seen[k] |= set(np.unique(classes(ref[k])).tolist())
    for k in ("sum", "mean", "min", "max"):
        assert seen[k] == {FINITE, PINF, NINF, NAN}, (k, seen[k])
    assert seen["var"] == seen["std"] == {FINITE, NAN}
    # theme 3: the all-NaN column is NaN in min and max of every row with edges; the second-segment case leaves finite extrema
    a, _, s = theme_all_nan(F)
    ref = multi_ref_nf(PTR, IDX, a["val"], a["x"])
    col = F // 3
    assert np.isnan(ref["min"][DEG > 0, col]).all() and np.isnan(ref["max"][DEG > 0, col]).all()
    ref = multi_ref_nf(PTR, IDX, s["val"], s["x"])
    b = int(PTR[ROW_1100])
    keep = np.r_[b:b + SEG_EDGES, b + 2 * SEG_EDGES:b + 1100]
    m = messages32(IDX, s["clean_val"], s["x"])
    assert np.array_equal(ref["min"][ROW_1100], m[keep].min(0)) and np.array_equal(ref["max"][ROW_1100], m[keep].max(0))
    assert np.isnan(ref["sum"][ROW_1100]).all() and np.isnan(ref["std"][ROW_1100]).all()
    # theme 4: the walk must form 0 * Inf = NaN; the reference has it at exactly the zeroed edges
    z = theme_zero_times_inf(F)[0]
    with np.errstate(invalid="ignore"):
        m = messages32(z["idx"], z["val"], z["x"])
    zeroed = np.flatnonzero(z["val"] == 0)
    assert len(zeroed) and np.isnan(m[zeroed]).all() and np.array_equal(np.flatnonzero(np.isnan(m).any(1)), zeroed)
    assert np.isinf(m).any() and (z["idx"][zeroed] == RESERVED).all()
