"""GPU: 16-bit features through gnnagg_gat_run_typed (Aggregator_GAT.run with torch.bfloat16 vin / vout).  bf16 -> fp32 is exact and the
kernels keep the fp32 path's weights, chains, denominators and division, so a bf16 x is compared EXACTLY with the fp32 run on x.float()
(same handle, same mode; newval too), and a bf16 y exactly with one round-to-nearest-even of that fp32 result.  The fp32 result itself is
held to the project's bound against the oracle (tests/test_gpu_parity.py: 1e-5 * (sum_e p_e |x_e| + |ref|)).  Whole outputs everywhere."""
import ctypes
import time

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-5   # the project's bound (tests/test_gpu_parity.py)
needs_extras = pytest.mark.skipif(not _lib.has_extras(), reason="second tier: needs libgnnagg_extras.so (GNNAGG_LIB)")

# heads x dhead: 16-, 8-, 4- and 2-byte bf16 lanes, heads narrower than a lane, more than one column tile (hubs through k_combine)
HD = [(1, 1), (1, 3), (1, 8), (1, 128), (1, 602), (4, 3), (4, 8), (8, 16), (8, 32), (2, 301)]


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print("\ntests/test_gpu_bf16_gat.py wall time: %.1f s" % (time.time() - t0))


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


def gat_scale(ptr, idx, att, x, heads, slope=0.2):
    """sum_e w_e |x_e| / sum_e w_e : the error scale of the normalised output (as in tests/test_gpu_parity.py)"""
    w = orc.gat_att(ptr, idx, att, heads, slope)  # normalised weights [E,H]
    V, F = len(ptr) - 1, x.shape[1]
    s = np.zeros((V, F))
    if len(idx):
        rows = np.repeat(np.arange(V), np.diff(ptr))
        np.add.at(s, rows, np.repeat(w, F // heads, axis=1).astype(np.float64) * np.abs(x[idx]))
    return s.astype(np.float32)


def assert_within(y, ref, scale, what):
    """|y - ref| <= RTOL * scale elementwise (as in tests/test_gpu_parity.py)"""
    err = np.abs(y.astype(np.float64) - ref.astype(np.float64))
    bound = RTOL * scale.astype(np.float64) + 1e-30
    bad = err > bound
    assert not bad.any(), "%s: %d elements outside the 1e-5 bound (worst ratio %.3g)" % (what, int(bad.sum()), float((err / bound).max()))


def make_agg(graph, ptr, idx, F):
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    if graph == "powerlaw":
        agg.schedule_balanced(16)   # hubs of more than 16 segments: segment workgroups, the in-kernel hub fold, k_combine on several tiles
        chunk, seg = agg.balanced_params()
        assert int(np.diff(ptr).max()) > 2 * chunk * seg   # hub rows exist
    return agg


@pytest.mark.parametrize("graph", ["uniform", "powerlaw"])
@pytest.mark.parametrize("H,D", HD)
def test_bf16_x_fp32_y_equals_the_fp32_run_and_meets_the_oracle_bound(graph, H, D):
    ptr, idx = GRAPHS[graph]()
    V, E, F = len(ptr) - 1, len(idx), H * D
    att = rand((V, H, 2), 2)
    xb, x32 = bf16_x(V, F, F + H)
    agg = make_agg(graph, ptr, idx, F)
    dx32, datt = dev(x32), dev(att)
    y32, nv32 = torch.full((V, F), 7.0, device=DEV), torch.full((E, H), 7.0, device=DEV)
    yb, nvb = torch.full((V, F), 7.0, device=DEV), torch.full((E, H), 7.0, device=DEV)
    agg.run(dx32, datt, y32, 128, "balanced", heads=H, newval=nv32)
    agg.run(xb, datt, yb, 128, "balanced", heads=H, newval=nvb)
    assert torch.equal(yb, y32) and torch.equal(nvb, nv32)
    # ... and without newval
    y32.fill_(7.0)
    yb.fill_(7.0)
    agg.run(dx32, datt, y32, 128, "balanced", heads=H)
    agg.run(xb, datt, yb, 128, "balanced", heads=H)
    assert torch.equal(yb, y32)
    ref = orc.gat_fused(ptr, idx, att, x32, H)
    assert_within(yb.cpu().numpy(), ref, gat_scale(ptr, idx, att, x32, H) + np.abs(ref), "bf16 x, fp32 y")
    empty = np.diff(ptr) == 0
    if graph == "uniform":
        assert empty.any()
    out = yb.cpu().numpy()[empty]
    assert np.all(out == 0) and not np.signbit(out).any()


@pytest.mark.parametrize("xdt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("H,D", HD)
def test_bf16_y_is_one_rounding_of_the_fp32_result(xdt, H, D):
    ptr, idx = powerlaw_graph()
    V, E, F = len(ptr) - 1, len(idx), H * D
    att = rand((V, H, 2), 3)
    xb, x32 = bf16_x(V, F, 100 + F + H)
    agg = make_agg("powerlaw", ptr, idx, F)
    dx32, datt = dev(x32), dev(att)
    x_in = xb if xdt == torch.bfloat16 else dx32
    y32, nv32 = torch.full((V, F), 7.0, device=DEV), torch.full((E, H), 7.0, device=DEV)
    agg.run(dx32, datt, y32, 128, "balanced", heads=H, newval=nv32)
    yb, nvb = torch.full((V, F), 7.0, device=DEV, dtype=torch.bfloat16), torch.full((E, H), 7.0, device=DEV)
    agg.run(x_in, datt, yb, 128, "balanced", heads=H, newval=nvb)
    assert torch.equal(yb, y32.to(torch.bfloat16)) and torch.equal(nvb, nv32)
    yb.fill_(7.0)
    agg.run(x_in, datt, yb, 128, "balanced", heads=H)
    assert torch.equal(yb, y32.to(torch.bfloat16))


def test_bf16_y_overflows_to_inf_where_the_rounding_does():
    """A GAT row is a convex combination of its sources, so only a fp32 x can leave bf16's range: entries between bf16's and fp32's
    largest finite values, zero attention terms and one-edge rows (weight exp(0) = 1, denominator 1: the fp32 result is x itself)."""
    ptr = np.array([0, 1, 2, 2, 3], np.int32)
    idx = np.array([1, 0, 3], np.int32)
    x = torch.tensor([[3.4e38, -3.4e38, 1.0, 3.39e38] * 2, [3.4e38] * 8, [5.0] * 8, [-2.0, 3.4e38] * 4])
    att = torch.zeros((4, 1, 2))
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), 8, 8)
    y32 = torch.full((4, 8), 7.0, device=DEV)
    agg.run(x.to(DEV), att.to(DEV), y32, 128, "balanced")
    yb = torch.full((4, 8), 7.0, device=DEV, dtype=torch.bfloat16)
    agg.run(x.to(DEV), att.to(DEV), yb, 128, "balanced")
    assert torch.isfinite(y32).all() and torch.equal(y32.cpu(), torch.stack([x[1], x[0], torch.zeros(8), x[3]]))
    expect = y32.to(torch.bfloat16)
    assert torch.isinf(expect).any() and torch.isfinite(expect).any()
    assert torch.equal(yb, expect) and torch.equal(torch.isinf(yb), torch.isinf(expect))


@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (4, 3)])
def test_scheduled_and_rows_paths(H, D):
    ptr, idx = powerlaw_graph()
    V, E, F = len(ptr) - 1, len(idx), H * D
    att = rand((V, H, 2), 4)
    xb, x32 = bf16_x(V, F, 7)
    dx32, datt = dev(x32), dev(att)
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    agg.schedule(gnc.Schedule.neighbor_grouping, [32])
    for fast in (1, 0):   # 1: the balanced order (calls without newval); 0: the user's groups in the restated order, on the plan kernel
        agg.set_option("fast_scheduled", fast)
        for with_nv in (False, True):
            nv32 = torch.full((E, H), 7.0, device=DEV) if with_nv else None
            nvb = torch.full((E, H), 7.0, device=DEV) if with_nv else None
            y32 = torch.full((V, F), 7.0, device=DEV)
            agg.run(dx32, datt, y32, 128, 1, heads=H, newval=nv32)
            for ydt in (torch.float32, torch.bfloat16):
                yb = torch.full((V, F), 7.0, device=DEV, dtype=ydt)
                agg.run(xb, datt, yb, 128, 1, heads=H, newval=nvb)
                assert torch.equal(yb, y32.to(ydt)), (fast, with_nv, ydt)
                if with_nv:
                    assert torch.equal(nvb, nv32)
    ref = orc.gat_fused(ptr, idx, att, x32, H)
    assert_within(y32.cpu().numpy(), ref, gat_scale(ptr, idx, att, x32, H) + np.abs(ref), "scheduled")
    # rows mode on a handle made through the reference-named surface maps to the balanced order (single head: its surface)
    if H == 1:
        at = gnc.gat_init(dev(ptr), dev(idx))
        y32 = torch.full((V, F), 7.0, device=DEV)
        gnc.gat_run(at, dx32, datt, y32, 128, 0)
        for ydt in (torch.float32, torch.bfloat16):
            yb = torch.full((V, F), 7.0, device=DEV, dtype=ydt)
            gnc.gat_run(at, xb, datt, yb, 128, 0)
            assert torch.equal(yb, y32.to(ydt))
        assert_within(y32.cpu().numpy(), ref, gat_scale(ptr, idx, att, x32, H) + np.abs(ref), "rows (fast_rows)")


@pytest.mark.parametrize("H,D", [(8, 16), (1, 100)])
def test_forced_partitions_run_the_chunked_plan(H, D):
    V, E, F = 600, 72000, H * D   # average degree 120: the 2-D blocked order's territory
    ptr, idx = gnc.graph.uniform_random_csr(V, E, seed=13)
    att = rand((V, H, 2), 5)
    xb, x32 = bf16_x(V, F, 11)
    dx32, datt = dev(x32), dev(att)
    blocked = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    blocked.set_option("partitions", 16)
    y_before = torch.full((V, F), 7.0, device=DEV)
    blocked.run(dx32, datt, y_before, 128, "balanced", heads=H)
    assert blocked.balanced_partitions() == 16
    plain = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    plain.set_option("partitions", 0)
    y_plain = torch.full((V, F), 7.0, device=DEV)
    plain.run(dx32, datt, y_plain, 128, "balanced", heads=H)
    assert plain.balanced_partitions() == 0
    for xin in (xb, dx32):
        for ydt in (torch.float32, torch.bfloat16):
            if xin is dx32 and ydt == torch.float32:
                continue
            yb = torch.full((V, F), 7.0, device=DEV, dtype=ydt)
            blocked.run(xin, datt, yb, 128, "balanced", heads=H)
            assert torch.equal(yb, y_plain.to(ydt))
    assert blocked.balanced_partitions() == 16   # the handle keeps its blocked order ...
    y_after = torch.full((V, F), 7.0, device=DEV)
    blocked.run(dx32, datt, y_after, 128, "balanced", heads=H)
    assert torch.equal(y_after, y_before)        # ... and fp32 calls keep using it


@needs_extras
@pytest.mark.parametrize("H,D", [(1, 100), (8, 16)])
def test_hubs_through_k_combine_on_one_tile(H, D):
    ptr, idx = powerlaw_graph()
    V, E, F = len(ptr) - 1, len(idx), H * D
    att = rand((V, H, 2), 6)
    xb, x32 = bf16_x(V, F, 12)
    agg = make_agg("powerlaw", ptr, idx, F)
    agg.set_option("inkernel_combine", 0)
    y32 = torch.full((V, F), 7.0, device=DEV)
    agg.run(dev(x32), dev(att), y32, 128, "balanced", heads=H)
    for ydt in (torch.float32, torch.bfloat16):
        yb = torch.full((V, F), 7.0, device=DEV, dtype=ydt)
        agg.run(xb, dev(att), yb, 128, "balanced", heads=H)
        assert torch.equal(yb, y32.to(ydt)), ydt
    ref = orc.gat_fused(ptr, idx, att, x32, H)
    assert_within(y32.cpu().numpy(), ref, gat_scale(ptr, idx, att, x32, H) + np.abs(ref), "k_combine")


@pytest.mark.parametrize("F", [3, 100, 128])
def test_unaligned_views(F):
    """X and Y as views at odd element offsets: narrower lanes, the same results; X is left as it was"""
    ptr, idx = powerlaw_graph()
    V, E = len(ptr) - 1, len(idx)
    att = dev(rand((V, 1, 2), 9))
    xb, x32 = bf16_x(V, F, 14)
    dx32 = dev(x32)
    agg = make_agg("powerlaw", ptr, idx, F)
    y32 = torch.full((V, F), 7.0, device=DEV)
    agg.run(dx32, att, y32, 128, "balanced")
    xbuf = torch.zeros(V * F + 1, device=DEV, dtype=torch.bfloat16)
    xv = xbuf[1:].view(V, F)
    xv.copy_(xb)
    xbuf32 = torch.zeros(V * F + 1, device=DEV)
    xv32 = xbuf32[1:].view(V, F)
    xv32.copy_(dx32)
    before = xbuf.clone()
    for ydt in (torch.float32, torch.bfloat16):
        ybuf = torch.full((V * F + 1,), 7.0, device=DEV, dtype=ydt)
        yv = ybuf[1:].view(V, F)
        agg.run(xv, att, yv, 128, "balanced")
        assert torch.equal(yv, y32.to(ydt)) and ybuf[0].item() == 7.0
        # aligned X with unaligned Y, unaligned X with aligned Y
        yv.fill_(7.0)
        agg.run(xb, att, yv, 128, "balanced")
        assert torch.equal(yv, y32.to(ydt)) and ybuf[0].item() == 7.0
        ya = torch.full((V, F), 7.0, device=DEV, dtype=ydt)
        agg.run(xv, att, ya, 128, "balanced")
        assert torch.equal(ya, y32.to(ydt))
    # a fp32 X at an odd 4-byte offset into a bf16 Y at an odd 2-byte offset
    ybuf = torch.full((V * F + 1,), 7.0, device=DEV, dtype=torch.bfloat16)
    yv = ybuf[1:].view(V, F)
    agg.run(xv32, att, yv, 128, "balanced")
    assert torch.equal(yv, y32.to(torch.bfloat16)) and ybuf[0].item() == 7.0
    assert torch.equal(xbuf, before)


@pytest.mark.parametrize("H,D", [(1, 128), (8, 16)])
def test_graph_capture_and_replay(H, D):
    ptr, idx = powerlaw_graph()
    V, E, F = len(ptr) - 1, len(idx), H * D
    att = dev(rand((V, H, 2), 10))
    xb, _ = bf16_x(V, F, 15)
    xb2, _ = bf16_x(V, F, 16)
    xb3, _ = bf16_x(V, F, 17)
    agg = make_agg("powerlaw", ptr, idx, F)
    for ydt in (torch.float32, torch.bfloat16):
        x = xb.clone()
        y = torch.empty((V, F), device=DEV, dtype=ydt)
        agg.run(x, att, y, 128, "balanced", heads=H)   # warm call: plan, scratch, counters
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            agg.run(x, att, y, 128, "balanced", heads=H)
        for xnew in (xb2, xb3):
            x.copy_(xnew)
            y.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            ref = torch.full((V, F), 7.0, device=DEV, dtype=ydt)
            agg.run(x, att, ref, 128, "balanced", heads=H)
            assert torch.equal(y, ref)


@pytest.mark.parametrize("H,D", [(1, 128), (8, 16)])
def test_arxiv_full_size(H, D):
    ptr_t, idx_t = gnc.graph.dataset("arxiv")
    V, F = ptr_t.numel() - 1, H * D
    agg = gnc.Aggregator_GAT(ptr_t.to(DEV), idx_t.to(DEV), F, F)
    att = dev(rand((V, H, 2), 18))
    xb, x32 = bf16_x(V, F, 19)
    y32 = torch.full((V, F), 7.0, device=DEV)
    agg.run(dev(x32), att, y32, 128, "balanced", heads=H)
    y16 = torch.full((V, F), 7.0, device=DEV, dtype=torch.bfloat16)
    agg.run(xb, att, y16, 128, "balanced", heads=H)
    assert torch.equal(y16, y32.to(torch.bfloat16))


def test_error_texts():
    ptr, idx = uniform_graph()
    V, F = len(ptr) - 1, 8
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    x = torch.zeros((V, F), device=DEV, dtype=torch.bfloat16)
    att = torch.zeros((V, 1, 2), device=DEV)
    y = torch.full((V, F), 7.0, device=DEV)
    L = gnc.lib()
    for xt, yt in ((2, _lib.DTYPE_F32), (_lib.DTYPE_BF16, -1)):
        rc = L.gnnagg_gat_run_typed(agg._h, ctypes.c_void_p(x.data_ptr()), xt, ctypes.c_void_p(att.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                    yt, F, 1, ctypes.c_float(0.2), _lib.MODE_BALANCED, None)
        assert rc == _lib.ERR_ARG and b"unknown dtype" in L.gnnagg_last_error()
    # the canonical CSR-order chains (fast_rows = 0, the status API's default) are fp32 only
    for yy in (y, torch.full((V, F), 7.0, device=DEV, dtype=torch.bfloat16)):
        with pytest.raises(_lib.GnnAggError) as e:
            agg.run(x, att, yy, 128, 0)
        assert e.value.code == _lib.ERR_ARG and "fast_rows" in str(e.value) and "x bf16" in str(e.value)
        torch.cuda.synchronize()
        assert (yy == 7.0).all()
    # an order the item kernels run (a locality schedule, restated) is fp32 only
    agg.set_option("fast_scheduled", 0)
    agg.schedule(gnc.Schedule.locality, [2])
    with pytest.raises(_lib.GnnAggError) as e:
        agg.run(x, att, y, 128, 1)
    assert e.value.code == _lib.ERR_ARG and "item kernels" in str(e.value) and "x bf16, y fp32" in str(e.value)
    y16 = torch.full((V, F), 7.0, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(_lib.GnnAggError) as e:
        agg.run(x.float(), att, y16, 128, 1)
    assert e.value.code == _lib.ERR_ARG and "x fp32, y bf16" in str(e.value)
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (y16 == 7.0).all()
    # the two-pass form and the gather probe are fp32 only: their C entry points take float *, a 16-bit tensor is refused before the call
    den = torch.zeros((V, 1), device=DEV)
    with pytest.raises(TypeError):
        agg.run_part(x, att, y, den, 1)
    with pytest.raises(TypeError):
        agg.run_part(x.float(), att, y16, den, 1)
    with pytest.raises(TypeError):
        agg.probe_gather(x, att)
    torch.cuda.synchronize()
