"""GPU: 16-bit features through gnnagg_gcn_run_typed (Aggregator_GCN.run with torch.bfloat16 vin / vout).  bf16 -> fp32 is exact and
the kernels keep the fp32 path's chains, so every comparison is exact: a bf16 x against the fp32 run on x.float() and against the oracle
in the order the run used; a bf16 y against one round-to-nearest-even of that fp32 result."""
import ctypes

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
needs_extras = pytest.mark.skipif(not _lib.has_extras(), reason="second tier: needs libgnnagg_extras.so (GNNAGG_LIB)")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def bf16_x(V, F, seed):
    """(bf16 device tensor, its fp32 widening as numpy)"""
    g = torch.Generator().manual_seed(seed)
    xb = torch.randn((V, F), generator=g).to(torch.bfloat16)
    return xb.to(DEV), xb.float().numpy()


def uniform_graph():
    return gnc.graph.uniform_random_csr(500, 9000, seed=5)   # ragged, with empty rows


def powerlaw_graph():
    p, i = gnc.graph.powerlaw_csr(4000, 100000, seed=9, alpha=1.1)   # rows with thousands of edges
    return p.numpy(), i.numpy()


GRAPHS = {"uniform": uniform_graph, "powerlaw": powerlaw_graph}


def balanced_ref(agg, ptr, idx, val, x32):
    ps, _, tg = agg.get_schedule("balanced")
    return orc.gcn_grouped(ps, tg, idx, val, x32, len(ptr) - 1, seg=agg.balanced_params()[1])


@pytest.mark.parametrize("graph", ["uniform", "powerlaw"])
@pytest.mark.parametrize("with_val", [True, False])
@pytest.mark.parametrize("F", [1, 3, 8, 32, 100, 128, 602])
def test_bf16_x_fp32_y_equals_the_fp32_run_and_the_oracle(graph, with_val, F):
    ptr, idx = GRAPHS[graph]()
    V, E = len(ptr) - 1, len(idx)
    val = rand(E, 2) if with_val else None
    xb, x32 = bf16_x(V, F, F)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), None if val is None else dev(val), F, F)
    if graph == "powerlaw":
        agg.schedule_balanced(16)   # hubs of more than 16 segments: segment workgroups and the in-kernel hub fold
        chunk, seg = agg.balanced_params()
        assert int(np.diff(ptr).max()) > 2 * chunk * seg
    dx32 = dev(x32)
    for red in ("sum", "max", "mean"):
        y32 = torch.full((V, F), 7.0, device=DEV)
        agg.run(dx32, y32, 512, "balanced", reduce=red)
        yb = torch.full((V, F), 7.0, device=DEV)
        agg.run(xb, yb, 512, "balanced", reduce=red)
        assert torch.equal(yb, y32), red
        if red == "sum":
            assert np.array_equal(yb.cpu().numpy(), balanced_ref(agg, ptr, idx, val, x32))
        elif red == "max":
            assert np.array_equal(yb.cpu().numpy(), orc.gcn_max(ptr, idx, val, x32))


@pytest.mark.parametrize("xdt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("F", [1, 3, 8, 100, 128, 602])
def test_bf16_y_is_one_rounding_of_the_fp32_result(xdt, F):
    ptr, idx = powerlaw_graph()
    V, E = len(ptr) - 1, len(idx)
    val = rand(E, 3)
    xb, x32 = bf16_x(V, F, 100 + F)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)
    agg.schedule_balanced(16)
    dx32 = dev(x32)
    x_in = xb if xdt == torch.bfloat16 else dx32
    for red in ("sum", "max", "mean"):
        y32 = torch.empty((V, F), device=DEV)
        agg.run(dx32, y32, 512, "balanced", reduce=red)
        yb = torch.full((V, F), 7.0, device=DEV, dtype=torch.bfloat16)
        agg.run(x_in, yb, 512, "balanced", reduce=red)
        assert torch.equal(yb, y32.to(torch.bfloat16)), red


@pytest.mark.parametrize("xdt", [torch.bfloat16, torch.float32])
def test_bf16_y_overflows_to_inf_where_the_rounding_does(xdt):
    """sums above bf16's largest finite value (but finite in fp32) round to inf, as torch's own conversion does"""
    ptr = np.array([0, 2, 3, 3, 4], np.int32)
    idx = np.array([0, 1, 0, 2], np.int32)
    val = np.array([1.0, 0.998, 1.998, 0.5], np.float32)
    x = torch.tensor([[2.0 ** 127] * 8, [2.0 ** 127] * 8, [1.0] * 8, [0.0] * 8]).to(torch.bfloat16)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), 8, 8)
    y32 = torch.empty((4, 8), device=DEV)
    agg.run(x.float().to(DEV), y32, 512, "balanced")
    yb = torch.empty((4, 8), device=DEV, dtype=torch.bfloat16)
    agg.run(x.to(DEV).to(xdt), yb, 512, "balanced")
    assert torch.isfinite(y32).all() and torch.isinf(yb[:2]).all() and torch.isfinite(yb[2:]).all()
    assert torch.equal(yb, y32.to(torch.bfloat16))


def test_scheduled_rows_and_partitioned_paths():
    ptr, idx = powerlaw_graph()
    V, E, F = len(ptr) - 1, len(idx), 128
    val = rand(E, 4)
    xb, x32 = bf16_x(V, F, 7)
    dx32 = dev(x32)
    # a neighbor-grouping schedule in the restated order, on the plan kernel
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)
    agg.set_option("fast_scheduled", 0)
    agg.schedule(gnc.Schedule.neighbor_grouping, [32])
    y32, yb = torch.empty((V, F), device=DEV), torch.empty((V, F), device=DEV)
    agg.run(dx32, y32, 512, 1)
    agg.run(xb, yb, 512, 1)
    assert torch.equal(yb, y32)
    ps, tg = orc.neighbor_grouping(ptr, 32)
    assert np.array_equal(yb.cpu().numpy(), orc.gcn_grouped(ps, tg, idx, val, x32, V, seg=agg.mode_params("scheduled")[1]))
    # the default fast_scheduled = 1: the balanced order
    agg.set_option("fast_scheduled", 1)
    agg.run(xb, yb, 512, 1)
    assert np.array_equal(yb.cpu().numpy(), balanced_ref(agg, ptr, idx, val, x32))
    # rows mode on a handle made through the reference-named surface maps to the balanced order
    at = gnc.gcn_init(dev(ptr), dev(idx), dev(val))
    gnc.gcn_run(at, dx32, y32, 512, 0)
    gnc.gcn_run(at, xb, yb, 512, 0)
    assert torch.equal(yb, y32)
    # ... and the canonical CSR-order chains (fast_rows = 0, the status API's default) are fp32 only
    with pytest.raises(_lib.GnnAggError) as e:
        agg.run(xb, yb, 512, 0)
    assert e.value.code == _lib.ERR_ARG and "fast_rows" in str(e.value)


def test_forced_partitions_run_the_chunked_plan():
    V, E, F = 600, 72000, 100   # average degree 120: the library would pick the 2-D blocked order
    ptr, idx = gnc.graph.uniform_random_csr(V, E, seed=13)
    val = rand(E, 5)
    xb, x32 = bf16_x(V, F, 11)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)
    agg.set_option("partitions", 16)
    y32 = torch.empty((V, F), device=DEV)
    agg.run(dev(x32), y32, 512, "balanced")
    assert agg.balanced_partitions() == 16
    for ydt in (torch.float32, torch.bfloat16):
        yb = torch.full((V, F), 7.0, device=DEV, dtype=ydt)
        agg.run(xb, yb, 512, "balanced")
        chunk = 64
        while chunk < 512 and chunk < 2 * (E // V):   # pick_chunk: the chunked plan's order, restated
            chunk *= 2
        ps, tg = orc.neighbor_grouping(ptr, chunk)
        ref = torch.from_numpy(orc.gcn_grouped(ps, tg, idx, val, x32, V, seg=16))
        assert torch.equal(yb.cpu(), ref.to(ydt))
    assert agg.balanced_partitions() == 16   # the handle keeps its blocked order for fp32 runs


@needs_extras
def test_hubs_through_k_combine():
    ptr, idx = powerlaw_graph()
    V, E, F = len(ptr) - 1, len(idx), 100
    val = rand(E, 6)
    xb, x32 = bf16_x(V, F, 12)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)
    agg.schedule_balanced(16)
    agg.set_option("inkernel_combine", 0)
    ref = balanced_ref(agg, ptr, idx, val, x32)
    for red in ("sum", "max"):
        y32 = torch.empty((V, F), device=DEV)
        agg.run(dev(x32), y32, 512, "balanced", reduce=red)
        for ydt in (torch.float32, torch.bfloat16):
            yb = torch.empty((V, F), device=DEV, dtype=ydt)
            agg.run(xb, yb, 512, "balanced", reduce=red)
            assert torch.equal(yb, y32.to(ydt)), (red, ydt)
        if red == "sum":
            assert np.array_equal(y32.cpu().numpy(), ref)


def test_relu_and_accumulate():
    ptr, idx = powerlaw_graph()
    V, E, F = len(ptr) - 1, len(idx), 128
    val = rand(E, 7)
    xb, x32 = bf16_x(V, F, 13)
    dx32 = dev(x32)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)
    agg.schedule_balanced(16)
    y32 = torch.empty((V, F), device=DEV)
    agg.run(dx32, y32, 512, "balanced", relu=True)
    for ydt in (torch.float32, torch.bfloat16):
        yb = torch.empty((V, F), device=DEV, dtype=ydt)
        agg.run(xb, yb, 512, "balanced", relu=True)
        assert torch.equal(yb, y32.to(ydt))
    y0 = torch.from_numpy(rand((V, F), 8)).to(DEV)
    ya, yb = y0.clone(), y0.clone()
    agg.run(dx32, ya, 512, "balanced", accumulate=True)
    agg.run(xb, yb, 512, "balanced", accumulate=True)
    assert torch.equal(yb, ya)
    ya, yb = y0.clone(), y0.clone()
    agg.run(dx32, ya, 512, "balanced", accumulate=True, relu=True)
    agg.run(xb, yb, 512, "balanced", accumulate=True, relu=True)
    assert torch.equal(yb, ya)
    with pytest.raises(_lib.GnnAggError) as e:
        agg.run(xb, torch.empty((V, F), device=DEV, dtype=torch.bfloat16), 512, "balanced", accumulate=True)
    assert e.value.code == _lib.ERR_ARG and "ACCUMULATE" in str(e.value)


@pytest.mark.parametrize("F", [3, 100, 128])
def test_unaligned_views(F):
    """X and Y as views at odd element offsets: narrower lanes, the same results; X is left as it was"""
    ptr, idx = powerlaw_graph()
    V, E = len(ptr) - 1, len(idx)
    val = rand(E, 9)
    xb, x32 = bf16_x(V, F, 14)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)
    agg.schedule_balanced(16)
    y32 = torch.empty((V, F), device=DEV)
    agg.run(dev(x32), y32, 512, "balanced")
    xbuf = torch.zeros(V * F + 1, device=DEV, dtype=torch.bfloat16)
    xv = xbuf[1:].view(V, F)
    xv.copy_(xb)
    before = xbuf.clone()
    for ydt in (torch.float32, torch.bfloat16):
        ybuf = torch.full((V * F + 1,), 7.0, device=DEV, dtype=ydt)
        yv = ybuf[1:].view(V, F)
        agg.run(xv, yv, 512, "balanced")
        assert torch.equal(yv, y32.to(ydt)) and ybuf[0].item() == 7.0
        # aligned X, unaligned Y and the other way round
        agg.run(xb, yv, 512, "balanced")
        assert torch.equal(yv, y32.to(ydt))
    assert torch.equal(xbuf, before)


def test_graph_capture_and_replay():
    ptr, idx = powerlaw_graph()
    V, E, F = len(ptr) - 1, len(idx), 128
    val = rand(E, 10)
    xb, _ = bf16_x(V, F, 15)
    xb2, _ = bf16_x(V, F, 16)
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), dev(val), F, F)
    agg.schedule_balanced(16)
    for ydt in (torch.float32, torch.bfloat16):
        y = torch.empty((V, F), device=DEV, dtype=ydt)
        agg.run(xb, y, 512, "balanced")   # warm-up: plan, scratch, counters
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            agg.run(xb, y, 512, "balanced")
        x_in = xb.clone()
        xb.copy_(xb2)
        y.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        ref = torch.empty_like(y)
        agg.run(xb, ref, 512, "balanced")
        assert torch.equal(y, ref)
        xb.copy_(x_in)


def test_arxiv_full_size():
    ptr_t, idx_t = gnc.graph.dataset("arxiv")
    V, F = ptr_t.numel() - 1, 128
    agg = gnc.Aggregator_GCN(ptr_t.to(DEV), idx_t.to(DEV), torch.ones(idx_t.numel(), device=DEV), F, F)
    xb, x32 = bf16_x(V, F, 17)
    y32, yb = torch.empty((V, F), device=DEV), torch.empty((V, F), device=DEV)
    agg.run(dev(x32), y32, 512, "balanced")
    agg.run(xb, yb, 512, "balanced")
    assert torch.equal(yb, y32)
    y16 = torch.empty((V, F), device=DEV, dtype=torch.bfloat16)
    agg.run(xb, y16, 512, "balanced")
    assert torch.equal(y16, y32.to(torch.bfloat16))


def test_error_texts():
    ptr, idx = uniform_graph()
    V, F = len(ptr) - 1, 8
    agg = gnc.Aggregator_GCN(dev(ptr), dev(idx), None, F, F)
    x = torch.zeros((V, F), device=DEV, dtype=torch.bfloat16)
    y = torch.zeros((V, F), device=DEV)
    L = gnc.lib()
    for xt, yt in ((2, _lib.DTYPE_F32), (_lib.DTYPE_BF16, -1)):
        rc = L.gnnagg_gcn_run_typed(agg._h, ctypes.c_void_p(x.data_ptr()), xt, ctypes.c_void_p(y.data_ptr()), yt, F, _lib.MODE_BALANCED,
                                    _lib.REDUCE_SUM, 0)
        assert rc == _lib.ERR_ARG and b"unknown dtype" in L.gnnagg_last_error()
    # an order the item kernels run (a locality schedule, restated) is fp32 only
    agg.set_option("fast_scheduled", 0)
    agg.schedule(gnc.Schedule.locality, [2])
    with pytest.raises(_lib.GnnAggError) as e:
        agg.run(x, y, 512, 1)
    assert e.value.code == _lib.ERR_ARG and "item kernels" in str(e.value)
    # run_with_nn is fp32 only: its C entry point takes float *, so a 16-bit tensor is refused before the call
    w, t = torch.zeros((F, 4), device=DEV), torch.zeros((V, 4), device=DEV)
    with pytest.raises(TypeError):
        agg.run_with_nn(x, y, w, t)
    with pytest.raises(TypeError):
        agg.run_with_nn(y, y.to(torch.bfloat16), w, t)
    torch.cuda.synchronize()
