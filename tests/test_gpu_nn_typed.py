"""GPU: gnnagg_gcn_run_with_nn_typed (Aggregator_GCN.run_with_nn_typed) -- the aggregation with the dense combine behind it, fp32 or bf16
features, every reduce and the fused ReLU.  One rule is checked everywhere: y is what the typed run writes, and transformed is the product
of y AS STORED -- the oracle's ascending-k fp32 chain for a fp32 y, the contract of gnnagg_matmul_nn_typed for a bf16 y (within
1e-5 . sum|y w| of the float64 product of the stored operands, exact on small integers; a bf16 transformed is one rounding of the fp32 one).
Outputs are pre-filled with NaN so that an element nobody wrote shows."""
import ctypes

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
# (y, weight, transformed) of the three accepted rows of the table; x is float32 or bfloat16 with each
PRODUCTS = [(F32, F32, F32), (BF16, BF16, F32), (BF16, BF16, BF16)]
SHAPES = [(128, 32), (64, 16), (256, 64), (100, 20), (30, 33), (602, 32), (7, 5)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def bf16_values(shape, seed):
    """seeded normal values that bf16 holds exactly, as a fp32 device tensor: the same x serves the fp32 and the bf16 runs"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(BF16).float().to(DEV)


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def hub_graph():
    """350 rows of 0 .. 6 edges, rows 11 / 180 / 349 with 4000 / 900 / 70 (the construction of test_nonfinite_host.gat_hub_graph),
    random edge values, chunk = 16: empty rows, short rows, a single-segment row (70), hubs of several segments (900, 4000)"""
    V = 350
    rng = np.random.default_rng(13)
    deg = rng.integers(0, 7, V)
    deg[11], deg[180], deg[349] = 4000, 900, 70
    ptr = np.zeros(V + 1, np.int32)
    ptr[1:] = np.cumsum(deg)
    idx = rng.integers(0, V, int(ptr[-1])).astype(np.int32)
    return ptr, idx, rand(len(idx), 2)


def powerlaw_graph():
    p, i = gnc.graph.powerlaw_csr(3000, 60000, seed=5, alpha=1.0)   # the graph of test_run_with_nn_fused_epilogue
    return p.numpy(), i.numpy(), rand(i.numel(), 2)


_GRAPHS = {}


def graph(name):
    """(ptr, idx, val) built once per session"""
    if name not in _GRAPHS:
        _GRAPHS[name] = {"hub": hub_graph, "powerlaw": powerlaw_graph}[name]()
    return _GRAPHS[name]


def aggregator(name, F, OUT):
    ptr, idx, val = graph(name)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, OUT)
    if name == "hub":
        agg.schedule_balanced(16)
        chunk, seg = agg.balanced_params()
        deg = np.diff(ptr)
        assert chunk == 16
        assert (deg > chunk * seg).any()                      # a hub with several segments
        assert ((deg > chunk) & (deg <= chunk * seg)).any()   # a single-segment row
        assert ((deg > 0) & (deg <= chunk)).any() and (deg == 0).any()   # short and empty rows
    return agg, len(ptr) - 1


def same(a, b):
    """equal where both are numbers, NaN where either is"""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all().item())


def check_product(y, w, t, t_ref_f32=None, rows=None, what=""):
    """contract 2 (fp32 y: bit-equal to the library GEMM of the stored y, the oracle's chain) or 3 (bf16 y: the bound against float64 of the
    stored operands; a bf16 transformed against one rounding of the fp32 one, t_ref_f32).  rows: the rows to check (default: all)."""
    if rows is None:
        rows = torch.ones(y.shape[0], dtype=torch.bool, device=DEV)
    if y.dtype == F32:
        assert torch.equal(t[rows], gnc.matmul_NN(y, w)[rows]), what
        return
    if t.dtype == BF16:
        assert torch.equal(t[rows], t_ref_f32.to(BF16)[rows]), what
        return
    y64, w64 = y.double(), w.double()
    err = (t.double() - y64 @ w64).abs()
    bound = 1e-5 * (y64.abs() @ w64.abs()) + 1e-30
    print("%s: max err / bound = %.3g" % (what, float((err[rows] / bound[rows]).max().item()) if rows.any() else 0.0))
    assert bool((err[rows] <= bound[rows]).all().item()), what


def run_all_products(agg, V, F, OUT, x32, w32, reduce, relu, what, oracle_chain):
    """contracts 1 - 3 for x in {fp32, bf16} x the three product rows"""
    for xdt in (F32, BF16):
        x = x32.to(xdt)
        t_f32 = None
        for ydt, wdt, tdt in PRODUCTS:
            tag = "%s x %s y %s t %s %s relu %d" % (what, xdt, ydt, tdt, reduce, relu)
            w = w32.to(wdt)
            y, t = nan_like((V, F), ydt), nan_like((V, OUT), tdt)
            agg.run_with_nn_typed(x, y, w, t, "balanced", reduce, relu)
            y2 = nan_like((V, F), ydt)
            agg.run(x, y2, 512, "balanced", reduce=reduce, relu=relu)
            assert torch.equal(y, y2), tag
            check_product(y, w, t, t_f32, what=tag)
            if ydt == F32 and oracle_chain:
                assert np.array_equal(t.cpu().numpy(), orc.matmul_nn(y.cpu().numpy(), w32.cpu().numpy())), tag
            if ydt == BF16 and tdt == F32:
                t_f32 = t


@pytest.mark.parametrize("F,OUT", SHAPES)
@pytest.mark.parametrize("name", ["hub", "powerlaw"])
def test_y_is_the_typed_run_and_transformed_its_product(name, F, OUT):
    """every accepted combination, reduce and ReLU setting: y equals run()'s, transformed the product of the stored y.  The oracle's chain is
    compared on the hub graph for every reduce and on the power-law graph for the sum (the library GEMM, bit-equal to it, everywhere)."""
    agg, V = aggregator(name, F, OUT)
    x32, w32 = bf16_values((V, F), F), bf16_values((F, OUT), 1000 + OUT)
    for reduce in ("sum", "mean", "max"):
        for relu in (False, True):
            run_all_products(agg, V, F, OUT, x32, w32, reduce, relu, name, name == "hub" or reduce == "sum")


def test_fp32_weights_need_not_be_bf16_values():
    """the fp32 product with arbitrary fp32 x and W, with and without ReLU: the oracle's chain on the stored y"""
    agg, V = aggregator("hub", 128, 32)
    x, w = rand((V, 128), 1), rand((128, 32), 3)
    for relu in (False, True):
        y, t = nan_like((V, 128), F32), nan_like((V, 32), F32)
        agg.run_with_nn_typed(dev(x), y, dev(w), t, relu=relu)
        y2 = nan_like((V, 128), F32)
        agg.run(dev(x), y2, 512, "balanced", relu=relu)
        assert torch.equal(y, y2)
        assert np.array_equal(t.cpu().numpy(), orc.matmul_nn(y.cpu().numpy(), w))


def test_small_integers_are_exact():
    """x, W integers in [-2, 2] and unit edge weights on uniform_random_csr(500, 9000, seed=5): the aggregate of a row is an integer of
    magnitude <= 2 * degree.  Rows of up to 128 edges (|y| <= 256: every such integer is a bf16 value) must be stored exactly; the graph also
    has a few longer rows (the longest 603 edges), whose stored y is the ONE rounding of the exact integer -- still an integer.  The product
    is taken from the stored y: every partial sum is an integer below 128 * 1206 * 2 < 2^24, so the fp32 transformed IS the int64 product
    of the stored y and W on every row, and the bf16 one its one rounding."""
    ptr, idx = gnc.graph.uniform_random_csr(500, 9000, seed=5)
    V, F, OUT = len(ptr) - 1, 128, 32
    deg = np.diff(ptr)
    small = torch.from_numpy(deg <= 128).to(DEV)
    assert int(small.sum().item()) > V // 2 and F * 2 * int(deg.max()) * 2 < 2 ** 24
    rng = np.random.default_rng(4)
    x, w = rng.integers(-2, 3, (V, F)), rng.integers(-2, 3, (F, OUT))
    y_int = np.zeros((V, F), np.int64)
    for r in range(V):
        y_int[r] = x[idx[ptr[r]:ptr[r + 1]]].sum(0)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), None, F, OUT)
    for relu in (False, True):
        yi = np.maximum(y_int, 0) if relu else y_int
        y_stored = torch.from_numpy(yi.astype(np.float32)).to(BF16)   # (|yi| < 2^24: the fp32 value is the integer)
        stored_int = y_stored.float().numpy().astype(np.int64)
        assert np.array_equal(stored_int[deg <= 128], yi[deg <= 128])
        t_int = torch.from_numpy(stored_int @ w).to(DEV)
        for xdt in (F32, BF16):
            dx, dw = dev(x.astype(np.float32)).to(xdt), dev(w.astype(np.float32)).to(BF16)
            y, t = nan_like((V, F), BF16), nan_like((V, OUT), F32)
            agg.run_with_nn_typed(dx, y, dw, t, relu=relu)
            assert agg.last_nn_path() == 1
            assert torch.equal(y, y_stored.to(DEV))
            assert torch.equal(y[small].double(), torch.from_numpy(yi).to(DEV)[small].double())
            assert torch.equal(t.double(), t_int.double())
            tb = nan_like((V, OUT), BF16)
            agg.run_with_nn_typed(dx, y, dw, tb, relu=relu)
            assert torch.equal(tb, t_int.float().to(BF16))


def test_last_nn_path_reports_what_the_launcher_took():
    """0 on a fresh handle; 1 (epilogue of the aggregation kernel) for the row widths one lane group spans, fp32 and bf16; 2 (separate GEMM)
    for F = 602, which takes several column tiles.  128 -> 64 and 256 -> 64 are 1 with the fp32 product and 2 with the bf16 product: measured on
    the arxiv-shaped input the bf16 epilogue with a W image above the 128 x 32 one loses to the back-to-back pair (88 against 72 us,
    182 against 115 us: profiles/nn_typed/bench_nn_typed.jsonl), so the launcher's rule leaves those to the bf16 GEMM.  So does a bf16 x of
    64 columns with a fp32 y: its 8-lane groups of 8 elements lost with the fp32 product (50.0 against 49.0 us at 64 -> 32) and are fused with
    the bf16 product only."""
    for F, OUT, want_f32, want_bf16 in ((128, 32, 1, 1), (64, 16, 1, 1), (602, 32, 2, 2), (128, 64, 1, 2), (256, 64, 1, 2)):
        agg, V = aggregator("powerlaw", F, OUT)
        assert agg.last_nn_path() == 0
        x32, w32 = bf16_values((V, F), 5), bf16_values((F, OUT), 6)
        for xdt in (F32, BF16):
            for ydt, wdt, tdt in PRODUCTS:
                for relu in (False, True):
                    agg.run_with_nn_typed(x32.to(xdt), nan_like((V, F), ydt), w32.to(wdt), nan_like((V, OUT), tdt), relu=relu)
                    want = want_f32 if ydt == F32 else want_bf16
                    if F == 64 and xdt == BF16 and ydt == F32:
                        want = 2
                    assert agg.last_nn_path() == want, (F, OUT, xdt, ydt, tdt, relu)
        agg.run_with_nn(x32, nan_like((V, F), F32), w32, nan_like((V, OUT), F32), 128, "balanced")
        assert agg.last_nn_path() == want_f32


def offset_view(shape, dtype, off, fill=None):
    """a contiguous [shape] view starting `off` elements into a larger buffer"""
    n = int(np.prod(shape))
    buf = torch.full((n + 16,), float("nan"), device=DEV, dtype=dtype)
    v = buf[off:off + n].view(shape)
    if fill is not None:
        v.copy_(fill)
    return v


@pytest.mark.parametrize("F,OUT", [(128, 32), (30, 33)])
@pytest.mark.parametrize("xoff", [1, 2, 4])
def test_unaligned_operands(F, OUT, xoff):
    """weight and transformed one element into their buffers (2-byte aligned bf16, 4-byte aligned fp32), y too, x offset so that the lanes
    narrow (align_class): contracts 1 - 3 as before, on whichever path the narrower geometry takes"""
    agg, V = aggregator("hub", F, OUT)
    x32, w32 = bf16_values((V, F), 7), bf16_values((F, OUT), 8)
    for xdt in (F32, BF16):
        x = offset_view((V, F), xdt, xoff, x32)
        t_f32 = None
        for ydt, wdt, tdt in PRODUCTS:
            w = offset_view((F, OUT), wdt, 1, w32)
            y, t = offset_view((V, F), ydt, 1), offset_view((V, OUT), tdt, 1)
            agg.run_with_nn_typed(x, y, w, t, relu=True)
            y2 = nan_like((V, F), ydt)
            agg.run(x32.to(xdt), y2, 512, "balanced", relu=True)
            assert torch.equal(y, y2), (xdt, ydt, tdt)
            check_product(y.clone(), w.clone(), t, t_f32, what="unaligned %s %s %s" % (xdt, ydt, tdt))
            if ydt == F32:
                assert np.array_equal(t.cpu().numpy(), orc.matmul_nn(y.cpu().numpy(), w32.cpu().numpy()))
            if ydt == BF16 and tdt == F32:
                t_f32 = t.clone()


@pytest.mark.parametrize("F,OUT", [(128, 32), (602, 32)])
def test_non_finite_features_stay_in_their_rows(F, OUT):
    """one source row of x NaN, one +Inf, with the ReLU: y equals the typed run's (NaN for NaN); transformed holds NaN only in rows whose y
    holds a NaN or an Inf, and contracts 2 / 3 hold in all the others"""
    agg, V = aggregator("hub", F, OUT)
    ptr, idx, _ = graph("hub")
    x32, w32 = bf16_values((V, F), 9), bf16_values((F, OUT), 10)
    short = np.flatnonzero(np.diff(ptr) <= 6)
    src = idx[ptr[short[5]]], idx[ptr[short[40]]]   # sources of two short rows (the hubs draw from nearly every row as well)
    x32[int(src[0])] = float("nan")
    x32[int(src[1])] = float("inf")
    for xdt in (F32, BF16):
        t_f32 = None
        for ydt, wdt, tdt in PRODUCTS:
            x, w = x32.to(xdt), w32.to(wdt)
            y, t = nan_like((V, F), ydt), nan_like((V, OUT), tdt)
            agg.run_with_nn_typed(x, y, w, t, relu=True)
            y2 = nan_like((V, F), ydt)
            agg.run(x, y2, 512, "balanced", relu=True)
            assert same(y, y2)
            good = torch.isfinite(y).all(1)
            assert bool(good.any().item()) and not bool(good.all().item())
            assert not bool(torch.isnan(t[good]).any().item())
            if ydt == F32:
                assert np.array_equal(t.cpu().numpy(), orc.matmul_nn(y.cpu().numpy(), w32.cpu().numpy()), equal_nan=True)
            else:
                yz = torch.where(good[:, None], y, torch.zeros_like(y))
                check_product(yz, w, t, t_f32, rows=good, what="non-finite %s %s" % (xdt, tdt))
            if ydt == BF16 and tdt == F32:
                t_f32 = t


def test_mean_with_empty_rows_bf16():
    """the 70-row graph of test_run_with_nn_mean_empty_rows in bf16: empty rows give y = 0 and transformed = 0"""
    V, F, OUT = 70, 64, 32
    ptr = np.zeros(V + 1, np.int32)
    ptr[10:] = 3
    idx = np.array([1, 2, 3], np.int32)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), None, F, OUT)
    x, w = bf16_values((V, F), 1).to(BF16), bf16_values((F, OUT), 3).to(BF16)
    for tdt in (F32, BF16):
        y, t = nan_like((V, F), BF16), nan_like((V, OUT), tdt)
        agg.run_with_nn_typed(x, y, w, t, reduce="mean")
        y2 = nan_like((V, F), BF16)
        agg.run(x, y2, 512, "balanced", reduce="mean")
        assert torch.equal(y, y2)
        empty = torch.ones(V, dtype=torch.bool, device=DEV)
        empty[9] = False
        assert bool((y[empty] == 0).all().item()) and bool((t[empty] == 0).all().item())
        assert bool((y[9] != 0).any().item()) and bool((t[9] != 0).any().item())
        check_product(y, w, t, gnc.matmul_NN(y, w, out_dtype=F32), what="mean, empty rows")


def test_orders_on_the_item_kernels():
    """a scheduled mode that runs on the item kernels refuses what the typed run refuses, with its text; an all-fp32 request without ReLU is
    run_with_nn's path there, with run_with_nn's bits"""
    ptr, idx = gnc.graph.uniform_random_csr(500, 9000, seed=5)
    V, F, OUT = len(ptr) - 1, 64, 16
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), None, F, OUT)
    agg.set_option("fast_scheduled", 0)
    agg.schedule(gnc.Schedule.locality, [2])
    x32, w32 = bf16_values((V, F), 11), bf16_values((F, OUT), 12)
    for xdt, ydt, wdt, tdt, relu in ((BF16, BF16, BF16, F32, False), (BF16, F32, F32, F32, False), (F32, BF16, BF16, BF16, True),
                                     (F32, F32, F32, F32, True)):
        with pytest.raises(_lib.GnnAggError) as e:
            agg.run_with_nn_typed(x32.to(xdt), nan_like((V, F), ydt), w32.to(wdt), nan_like((V, OUT), tdt), 1, "sum", relu)
        assert e.value.code == _lib.ERR_ARG and "gnnagg_gcn_run_typed" in str(e.value) and "item kernels" in str(e.value)
    y, t = nan_like((V, F), F32), nan_like((V, OUT), F32)
    agg.run_with_nn_typed(x32, y, w32, t, 1)
    y2, t2 = nan_like((V, F), F32), nan_like((V, OUT), F32)
    agg.run_with_nn(x32, y2, w32, t2, 128, 1)
    assert torch.equal(y, y2) and torch.equal(t, t2)
    assert agg.last_nn_path() == 2
    torch.cuda.synchronize()


@pytest.mark.parametrize("F,OUT", [(128, 32), (602, 32)])
def test_the_old_entry_point_is_unchanged(F, OUT):
    """run_with_nn (fp32) and the all-fp32, no-ReLU run_with_nn_typed: the same bits, y and transformed"""
    agg, V = aggregator("powerlaw", F, OUT)
    x, w = dev(rand((V, F), 1)), dev(rand((F, OUT), 3))
    y, t = nan_like((V, F), F32), nan_like((V, OUT), F32)
    agg.run_with_nn(x, y, w, t, 128, "balanced")
    y2, t2 = nan_like((V, F), F32), nan_like((V, OUT), F32)
    agg.run_with_nn_typed(x, y2, w, t2)
    assert torch.equal(y, y2) and torch.equal(t, t2)
    assert np.array_equal(t.cpu().numpy(), orc.matmul_nn(y.cpu().numpy(), w.cpu().numpy()))
    L = gnc.lib()
    rc = L.gnnagg_gcn_run_with_nn_typed(agg._h, ctypes.c_void_p(x.data_ptr()), 0, ctypes.c_void_p(y.data_ptr()), 0, ctypes.c_void_p(w.data_ptr()), 0,
                                        ctypes.c_void_p(t.data_ptr()), 0, F, OUT, _lib.MODE_BALANCED, _lib.REDUCE_SUM, _lib.FLAG_ACCUMULATE)
    assert rc == _lib.ERR_ARG
