"""GPU: gnnagg_gcn_run_multi (Aggregator_GCN.run_multi) -- sum / mean / min / max / var / std of a row's messages from one gather, times
the degree scalers -- on the fixture of tests/test_multi_aggr_host.py, one feature width per case of the kernel's dispatch switch.
The references are computed once per (width, feature set, val) and shared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_multi_aggr_host import (AGGRS, BOUNDS, CENSUS_F, LONG_EDGES, SCALERS, fixture_graph, fixture_val, fixture_x, multi_chain32,
                                  multi_layout, multi_ref, multi_width, scaler64, worst_ratio)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
ALL_F = sorted(set(CENSUS_F) | {1, 3, 5, 100, 128, 602, 1024})   # one width per case of the switch, and the widths the census must hold
FEW_F = [5, 101, 128, 602, 1024]                                # a scalar and a packed geometry of one fragment and of several
PTR, IDX, N_SRC = fixture_graph()
V, E = len(PTR) - 1, len(IDX)
DEG = np.diff(PTR)
SHORT, HAS = DEG <= LONG_EDGES, DEG > 0
DELTA = gnc.pna_delta(PTR) if hasattr(gnc, "pna_delta") else 1.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def handle(val=None, idx=None):
    return gnc.Aggregator_GCN(dev(PTR), dev(IDX if idx is None else idx), None if val is None else dev(val))


@functools.lru_cache(maxsize=None)
def shared_handle(with_val):
    return handle(fixture_val() if with_val else None)


@functools.lru_cache(maxsize=None)
def refs(F, mean, with_val):
    """(float64 reference, float32 restatement) of the fixture at width F: computed once, never written"""
    x, val = fixture_x(F, mean), (fixture_val() if with_val else None)
    return multi_ref(PTR, IDX, val, x), multi_chain32(PTR, IDX, val, x)


def run(at, x, aggrs=AGGRS, scalers=SCALERS, ydtype=torch.float32, delta=DELTA):
    y = torch.full((V, multi_width(aggrs, scalers, x.shape[1])), 7.0, device=DEV, dtype=ydtype)
    at.run_multi(x, y, aggrs=aggrs, scalers=scalers, delta=delta)
    return y


def blocks(y, aggrs, scalers, F):
    """{(scaler, aggr): numpy block}"""
    a = y.float().cpu().numpy() if y.dtype == BF else y.cpu().numpy()
    return {k: a[:, s] for k, s in multi_layout(aggrs, scalers, F).items()}


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def np_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check_against_refs(blk, F, mean, with_val, rows=slice(None), exact_rows=SHORT):
    """the identity blocks of a fp32 call against the references: min / max ==, sum / mean bit-equal to the restatement on exact_rows and
    inside the bar everywhere, var / std inside their bounds"""
    ref, c32 = refs(F, mean, with_val)
    sel = np.zeros(V, bool)
    sel[rows] = True
    assert np.array_equal(blk[("identity", "min")][sel], ref["min"][sel]) and np.array_equal(blk[("identity", "max")][sel], ref["max"][sel])
    ex = sel & exact_rows
    for k in ("sum", "mean"):
        assert np.array_equal(np_bits(blk[("identity", k)][ex]), np_bits(c32[k][ex])), "%s: not the float32 chain on the short rows" % k
    for k in ("sum", "mean", "var", "std"):
        ratio = worst_ratio(blk[("identity", k)][sel], ref[k][sel], BOUNDS[k](ref)[sel])
        print("F = %d, mean %g, val %s: %s worst |y - ref| / bound = %.4f" % (F, mean, with_val, k, ratio))
        assert ratio <= 1.0, (k, ratio)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", ALL_F)
def test_exactness_with_every_mask_set(F):
    y = run(shared_handle(True), dev(fixture_x(F)))
    assert bool(torch.isfinite(y).all())
    check_against_refs(blocks(y, AGGRS, SCALERS, F), F, 0.0, True)


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FEW_F)
@pytest.mark.parametrize("with_val", [False, True])
def test_var_and_std_bounds_under_cancellation(F, with_val):
    """features of mean 100: S2 / d and mean^2 agree in their leading digits"""
    y = run(shared_handle(with_val), dev(fixture_x(F, 100.0)), scalers=("identity",))
    blk = blocks(y, AGGRS, ("identity",), F)
    check_against_refs(blk, F, 100.0, with_val)
    assert (blk[("identity", "var")] >= 0).all() and np.isfinite(blk[("identity", "std")]).all()


@pytest.mark.parametrize("F", [3, 128])
def test_var_is_clamped_on_rows_of_identical_messages(F):
    """every message 1000.25: the variance is 0, and S2 / d - mean^2 in fp32 lands on either side of it"""
    x = torch.full((N_SRC, F), 1000.25, device=DEV)
    y = run(shared_handle(False), x, aggrs=("mean", "var", "std"), scalers=("identity",))
    blk = blocks(y, ("mean", "var", "std"), ("identity",), F)
    var, std = blk[("identity", "var")], blk[("identity", "std")]
    assert np.isfinite(var).all() and np.isfinite(std).all()
    assert not np.signbit(var).any() and not np.signbit(std).any()  # (no -0.0 either: the clamp d < 0 ? 0 : d would keep one)
    assert (var <= 4e-5 * 1000.25 ** 2).all()                       # the bound with sum m^2 / d = 1000.25^2 and a reference of 0
    assert np.abs(blk[("identity", "mean")][HAS] - 1000.25).max() <= 1e-5 * 1000.25


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FEW_F)
def test_a_block_does_not_depend_on_the_other_blocks(F):
    at, x = shared_handle(True), dev(fixture_x(F))
    full = run(at, x)
    lay = multi_layout(AGGRS, SCALERS, F)
    for a in AGGRS:
        one = run(at, x, aggrs=(a,), scalers=("identity",))
        assert same_bits(one, full[:, lay[("identity", a)]].contiguous()), a
    for s in SCALERS:
        one = run(at, x, aggrs=AGGRS, scalers=(s,))
        want = torch.cat([full[:, lay[(s, a)]] for a in AGGRS], 1)
        assert same_bits(one, want), s
    pair = run(at, x, aggrs=("max", "sum"), scalers=("attenuation", "identity"))       # names in any order: blocks in bit order
    want = torch.cat([full[:, lay[(s, a)]] for s in ("identity", "attenuation") for a in ("sum", "max")], 1)
    assert same_bits(pair, want)


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FEW_F)
@pytest.mark.parametrize("with_val", [False, True])
def test_against_the_existing_reductions(F, with_val):
    at, x = shared_handle(with_val), dev(fixture_x(F))
    blk = blocks(run(at, x, aggrs=("sum", "min", "max"), scalers=("identity",)), ("sum", "min", "max"), ("identity",), F)
    y = torch.empty((V, F), device=DEV)
    at.run(x, y, reduce="max")
    assert np.array_equal(blk[("identity", "max")][HAS], y.cpu().numpy()[HAS])
    at.run(-x, y, reduce="max")
    assert np.array_equal(blk[("identity", "min")][HAS], -y.cpu().numpy()[HAS])
    at.run(x, y, reduce="sum")
    ref, _ = refs(F, 0.0, with_val)
    assert worst_ratio(blk[("identity", "sum")], y.cpu().numpy().astype(np.float64), BOUNDS["sum"](ref)) <= 1.0


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FEW_F)
@pytest.mark.parametrize("ydtype", [torch.float32, BF])
def test_scaler_blocks_are_the_identity_block_times_the_scaler(F, ydtype):
    """1e-6 (fp32 y): logf at <= 1 ulp (what the HIP math API documents for logf), one correctly rounded division and one multiply -- under
    4 * 2^-24 = 2.4e-7.  2^-8 (bf16 y): one rounding to 8 significant bits (2^-9) on top of that, against the identity block of the
    fp32-y call."""
    at, x = shared_handle(True), dev(fixture_x(F))
    ident = blocks(run(at, x), AGGRS, SCALERS, F)
    blk = blocks(run(at, x, ydtype=ydtype), AGGRS, SCALERS, F)
    tol = 1e-6 if ydtype == torch.float32 else 2.0 ** -8
    for s in ("amplification", "attenuation"):
        sc = scaler64(s, DEG, DELTA)[:, None]
        for a in AGGRS:
            want = ident[("identity", a)].astype(np.float64) * sc
            err = np.abs(blk[(s, a)].astype(np.float64) - want)
            assert (err <= tol * np.abs(want)).all(), (s, a, float((err / np.maximum(np.abs(want), 1e-300)).max()))
    for k, b in blk.items():
        assert not np_bits(b[~HAS]).any(), "%s: a row without edges is not +0" % (k,)


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 100, 128, 256, 1024])
def test_the_four_dtype_pairs(F):
    at = shared_handle(True)
    xb = dev(fixture_x(F)).to(BF)
    xw = xb.float()                                                  # the widened features: what the bf16 call computes on
    y_ff, y_bf = run(at, xw), run(at, xb)
    assert same_bits(y_bf[dev(SHORT)], y_ff[dev(SHORT)]), "bf16 x is not the fp32 call on the widened x (short rows)"
    val = fixture_val()
    xw_np = xw.cpu().numpy()
    ref = multi_ref(PTR, IDX, val, xw_np)
    for name, y in (("fp32 x", y_ff), ("bf16 x", y_bf)):
        blk = blocks(y, AGGRS, SCALERS, F)
        assert np.array_equal(blk[("identity", "min")], ref["min"]) and np.array_equal(blk[("identity", "max")], ref["max"])
        for k in ("sum", "mean", "var", "std"):
            ratio = worst_ratio(blk[("identity", k)], ref[k], BOUNDS[k](ref))
            assert ratio <= 1.0, (name, k, ratio)
    assert same_bits(run(at, xw, ydtype=BF), y_ff.to(BF)), "bf16 y is not one RNE rounding of the fp32 y (fp32 x)"
    assert same_bits(run(at, xb, ydtype=BF), y_bf.to(BF)), "bf16 y is not one RNE rounding of the fp32 y (bf16 x)"


# 7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 128])
def test_val_present_absent_and_replaced(F):
    x = dev(fixture_x(F))
    at = handle(None)
    y_none = run(at, x)
    check_against_refs(blocks(y_none, AGGRS, SCALERS, F), F, 0.0, False)
    ones = torch.ones(E, device=DEV)
    at.updateval(ones)
    assert same_bits(run(at, x), y_none), "an all-ones val does not give the bits of the call without val"
    at.updateval(dev(fixture_val()))                                 # the next call follows the new values
    y_val = run(at, x)
    check_against_refs(blocks(y_val, AGGRS, SCALERS, F), F, 0.0, True)
    assert same_bits(y_val, run(shared_handle(True), x))
    at.updateval(None)
    assert same_bits(run(at, x), y_none)


# 8 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 128])
def test_infinities_follow_ieee_and_reach_only_the_rows_that_gather_them(F):
    at = shared_handle(False)
    x_np = fixture_x(F).copy()
    clean = run(at, dev(x_np), scalers=("identity",)).cpu().numpy()
    a, b, col = 3, 17, F // 2
    x_np[a, col], x_np[b, col] = np.inf, -np.inf
    got = run(at, dev(x_np), scalers=("identity",)).cpu().numpy()
    lay = multi_layout(AGGRS, ("identity",), F)
    has_a = np.array([a in IDX[PTR[r]:PTR[r + 1]] for r in range(V)])
    has_b = np.array([b in IDX[PTR[r]:PTR[r + 1]] for r in range(V)])
    assert (has_a & ~has_b).any() and (has_b & ~has_a).any() and (has_a & has_b).any() and (~has_a & ~has_b & HAS).any()
    ref = multi_ref(PTR, IDX, None, x_np)                             # float64 over the same messages: plain IEEE
    hit = np.zeros_like(got, bool)
    for k in AGGRS:
        hit[np.ix_(has_a | has_b, [lay[("identity", k)].start + col])] = True
    for k in ("sum", "mean", "min", "max"):
        g = got[:, lay[("identity", k)]][:, col][has_a | has_b]
        w = ref[k][:, col][has_a | has_b]
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(w)], w[~np.isnan(w)].astype(np.float32)), k
    s = got[:, lay[("identity", "sum")]][:, col]
    assert np.isnan(s[has_a & has_b]).all() and (s[has_a & ~has_b] == np.inf).all() and (s[has_b & ~has_a] == -np.inf).all()
    assert np.array_equal(np_bits(got)[~hit], np_bits(clean)[~hit]), "a value changed that no infinity reaches"


# 9 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FEW_F)
@pytest.mark.parametrize("xdtype,ydtype", [(torch.float32, torch.float32), (BF, BF)])
def test_memory_canaries_offsets_and_repeats(F, xdtype, ydtype):
    at = shared_handle(True)
    x = dev(fixture_x(F)).to(xdtype)
    y0 = run(at, x, ydtype=ydtype)
    assert same_bits(run(at, x, ydtype=ydtype), y0), "two calls differ"
    assert same_bits(run(handle(fixture_val()), x, ydtype=ydtype), y0), "a fresh handle differs from the reused one"
    # x and y at element offset 1 (no 16-byte alignment, for bf16 not even 4-byte), canary words around y
    W = y0.shape[1]
    xbuf = torch.zeros(N_SRC * F + 9, device=DEV, dtype=xdtype)
    xo = xbuf[1:1 + N_SRC * F].view(N_SRC, F)
    xo.copy_(x)
    ybuf = torch.full((V * W + 10,), 7.0, device=DEV, dtype=ydtype)
    yo = ybuf[1:1 + V * W].view(V, W)
    assert xo.data_ptr() % 16 != 0 and yo.data_ptr() % 16 != 0
    at.run_multi(xo, yo, aggrs=AGGRS, scalers=SCALERS, delta=DELTA)
    assert same_bits(yo.contiguous(), y0), "the bits depend on the alignment of x / y"
    assert bool((ybuf[:1] == 7.0).all()) and bool((ybuf[1 + V * W:] == 7.0).all()), "a canary word around y was written"


def test_a_source_row_that_no_edge_names_is_never_read_into_a_result():
    F, u = 128, 11
    idx = IDX.copy()
    idx[idx == u] = u + 1
    at = handle(fixture_val(), idx)
    x = fixture_x(F).copy()
    want = run(at, dev(x))
    x[u] = np.nan
    got = run(at, dev(x))
    assert bool(torch.isfinite(got).all()) and same_bits(got, want)


# 10 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,xdtype", [(128, torch.float32), (602, BF)])
def test_a_captured_call_replays_on_rewritten_features(F, xdtype):
    at = handle(fixture_val())
    x = dev(fixture_x(F)).to(xdtype)
    y = torch.full((V, multi_width(AGGRS, SCALERS, F)), 7.0, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        at.run_multi(x, y, aggrs=AGGRS, scalers=SCALERS, delta=DELTA)      # the first call of the shape: plan and scratch
        side.synchronize()
        eager = y.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):                              # the second: nothing but launches, in a line
            at.run_multi(x, y, aggrs=AGGRS, scalers=SCALERS, delta=DELTA)
        y.fill_(7.0)
        g.replay()
        side.synchronize()
        assert same_bits(y, eager)
        x.mul_(0.5)                                                         # rewritten in place: the replay follows
        g.replay()
        side.synchronize()
        replayed = y.clone()
        assert not same_bits(replayed, eager)
        at.run_multi(x, y, aggrs=AGGRS, scalers=SCALERS, delta=DELTA)
        side.synchronize()
        assert same_bits(y, replayed)
    torch.cuda.current_stream().wait_stream(side)


# 11 -----------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_y_alone():
    L = gnc.lib()
    F = 8
    gcn, gat = handle(None), gnc.Aggregator_GAT(dev(PTR), dev(IDX))
    x = dev(fixture_x(F))
    y = torch.full((V, 18 * F), 7.0, device=DEV)
    px, py = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr())
    f32 = _lib.DTYPE_F32
    cases = [
        ((gat._h, px, f32, py, f32, F, 63, 7, 1.0), "not a GCN aggregator"),
        ((gcn._h, None, f32, py, f32, F, 63, 7, 1.0), "d_x"),
        ((gcn._h, px, f32, None, f32, F, 63, 7, 1.0), "d_y"),
        ((gcn._h, px, 2, py, f32, F, 63, 7, 1.0), "x_dtype 2"),
        ((gcn._h, px, f32, py, -1, F, 63, 7, 1.0), "y_dtype -1"),
        ((gcn._h, px, f32, py, f32, 0, 63, 7, 1.0), "feat = 0"),
        ((gcn._h, px, f32, py, f32, 1025, 1, 1, 1.0), "feat = 1025"),
        ((gcn._h, px, f32, py, f32, F, 0, 7, 1.0), "aggr_mask = 0"),
        ((gcn._h, px, f32, py, f32, F, 64, 7, 1.0), "aggr_mask = 64"),
        ((gcn._h, px, f32, py, f32, F, 63, 0, 1.0), "scaler_mask = 0"),
        ((gcn._h, px, f32, py, f32, F, 63, 8, 1.0), "scaler_mask = 8"),
        ((gcn._h, px, f32, py, f32, F, 63, 3, 0.0), "delta"),
        ((gcn._h, px, f32, py, f32, F, 63, 4, -1.0), "delta"),
        ((gcn._h, px, f32, py, f32, F, 63, 6, float("nan")), "delta"),
        ((gcn._h, px, f32, py, f32, F, 63, 2, float("inf")), "delta"),
    ]
    for args, text in cases:
        assert L.gnnagg_gcn_run_multi(*args) == _lib.ERR_ARG, text
        msg = L.gnnagg_last_error().decode()
        assert "gnnagg_gcn_run_multi" in msg and text in msg, (text, msg)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), "a refused call wrote to y"
    # delta is not looked at where only the identity scaler is selected
    assert L.gnnagg_gcn_run_multi(gcn._h, px, f32, py, f32, F, 63, 1, float("nan")) == _lib.OK
    torch.cuda.synchronize()


def test_the_wrapper_raises_before_the_library_is_reached():
    at = handle(None)
    x = dev(fixture_x(8))
    y = torch.empty((V, 4 * 8), device=DEV)
    at.run_multi(x, y)                                                       # the defaults: mean, min, max, std x identity
    with pytest.raises(ValueError):
        at.run_multi(x, torch.empty((V, 3 * 8), device=DEV))
    with pytest.raises(ValueError):
        at.run_multi(x, torch.empty((V + 1, 4 * 8), device=DEV))
    with pytest.raises(ValueError):
        at.run_multi(x, y, aggrs=("mean", "min", "max", "median"))
    with pytest.raises(ValueError):
        at.run_multi(x, y, aggrs=("mean", "min", "max", "max"))
    with pytest.raises(ValueError):
        at.run_multi(x, y, scalers=("linear",))
    with pytest.raises(ValueError):
        at.run_multi(x, torch.empty((V, 8 * 8), device=DEV), scalers=("identity", "amplification"))      # no delta
    with pytest.raises(ValueError):
        at.run_multi(x, torch.empty((V, 8 * 8), device=DEV), scalers=("identity", "amplification"), delta=0.0)
    with pytest.raises(TypeError):
        at.run_multi(x.double(), y)
    with pytest.raises(ValueError):
        at.run_multi(x.cpu(), y)
    with pytest.raises(ValueError):
        at.run_multi(x[:, 0], y)
    y2 = torch.empty((V, 4 * 8), device=DEV)
    gnc.gcn_run_multi(at, x, y2)
    assert same_bits(y, y2)
