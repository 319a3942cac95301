"""GPU: every lane geometry the kernel dispatchers can select, against float64 (the census of tests/geometry_census.py).

The suite's other GPU files are deep on graphs, row lengths, logits, non-finite values and sizes, at the benchmark's shapes; this file is
wide on SHAPES: one small case per (VEC, GROUP, ntiles) of pick_geometry / typed_geometry and per (GROUP, NF) / NF of gatv2_geometry,
through every call that dispatches on them.  The judges are the project's own:
  * GCN: the integer data of tests/test_gpu_large.py (features in [-8, 8], val in [1, 3], degree x 24 < 2^24): sum / mean / max / ReLU are
    exact in any association, the whole NaN-prefilled output EQUALS a float64 gather-and-reduce; a bf16 y is one rounding of the fp32 y
    (balanced mode on the plan kernels, rows mode, and the item kernels + k_combine on a restated locality schedule);
  * run_with_nn_typed: y equal to run() on the same handle, the product under check_product of tests/test_gpu_nn_typed.py;
  * GAT: orc.gat_fused under assert_within / gat_scale of tests/test_gpu_bf16_gat.py; a bf16 x bit-equal to the fp32 run on its widening;
  * gnnagg_pack_rows: equal to x[ids];
  * run_v2 / run_dot: run_pairs_and_judge of tests/test_gpu_gatv2.py and tests/test_gpu_dot_attn.py (gatv2_bound / dot_attn_bound, the whole
    output, empty rows +0, a bf16 y one rounding), and unaligned views bit-equal to the aligned run (the x_aligned = 0 path).
All operands are torch allocations, asserted 16-byte aligned, so shape and dtype alone select the geometry; every case prints the tuple
the census expects.  profiles/geometry_census/ holds the kernel names one traced run of this file launched."""
import ctypes
import time

import numpy as np
import pytest
import torch

import geometry_census as gc
import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from oracle import oracle as orc
from test_gatv2_host import gatv2_ref
from test_gpu_bf16_gat import DEV, assert_within, bf16_x, dev, gat_scale, rand
from test_gpu_dot_attn import pitched
from test_gpu_dot_attn import run_pairs_and_judge as judge_dot
from test_gpu_gatv2 import att_vec, bf16_pair, full, judge_block, threshold_graph
from test_gpu_gatv2 import run_pairs_and_judge as judge_v2
from test_gpu_large import Graph, gcn_block, gen, ints, poisoned
from test_gpu_nn_typed import PRODUCTS, check_product

pytestmark = pytest.mark.gpu

F32, B16 = torch.float32, torch.bfloat16
THRESHOLDS = gnc.Aggregator_GAT.GATV2_THRESHOLDS
BATCH = THRESHOLDS[0]
CHUNK = 16   # schedule_balanced(16): rows above 16 edges are chunked, above 16 x 16 they are hubs of several segments


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print("\ntests/test_gpu_geometry_census.py wall time: %.1f s" % (time.time() - t0))


def aligned(*tensors):
    assert all(t.data_ptr() % 16 == 0 for t in tensors), "the census assumes 16-byte aligned operands"


# ------------------------------------------------------------------------------------------------------------ the GCN / GAT graph
_GRAPH = []


def census_graph():
    """a power-law graph of a thousand rows (hubs of several segments, single-segment rows, short rows, an empty row) with an empty row
    and a one-edge row appended: (ptr, idx) as numpy, built once"""
    if not _GRAPH:
        p, i = gnc.graph.powerlaw_csr(1000, 12000, seed=9, alpha=1.1)
        ptr, idx = p.numpy().astype(np.int64), i.numpy().astype(np.int32)
        ptr = np.concatenate([ptr, [ptr[-1], ptr[-1] + 1]]).astype(np.int32)
        idx = np.concatenate([idx, [3]]).astype(np.int32)
        _GRAPH.append((ptr, idx))
    return _GRAPH[0]


def assert_row_classes(agg, ptr):
    """what make_agg of tests/test_gpu_bf16_gat.py asserts, and the other classes the plan kernels distinguish"""
    chunk, seg = agg.balanced_params()
    deg = np.diff(ptr)
    assert chunk == CHUNK
    assert int(deg.max()) > 2 * chunk * seg                       # hubs: segment workgroups, the hub fold, the combine kernels
    assert ((deg > chunk) & (deg <= chunk * seg)).any()           # single-segment rows
    assert ((deg > 1) & (deg <= chunk)).any()                     # short rows
    assert deg[-2] == 0 and deg[-1] == 1 and (deg[:-2] == 0).any()   # empty rows and a one-edge row


# ------------------------------------------------------------------------------------------------------------ 1. GCN
GCN_FEATS = sorted(set(gc.GCN_F32) | set(gc.GCN_BF16))


def gcn_want(total, deg, reduce, relu, ydt):
    """what Y must hold bit for bit (tests/test_gpu_large.py gcn_expect): total = the exact float64 sum (or max)"""
    want = total.float()
    if reduce == "mean":
        want = want / deg.clamp(min=1).float()[:, None]
    if relu:
        want = want.clamp_min(0.0)
    return want.to(ydt)


@pytest.mark.parametrize("F", GCN_FEATS)
def test_gcn_every_geometry_is_exact_on_integer_data(F):
    ptr, idx = census_graph()
    G = Graph(ptr, idx, len(ptr) - 1)   # (asserts degree x 24 < 2^24)
    V, E = G.V, G.E
    g = gen(100 + F)
    x32 = ints((V, F), g)
    xb = x32.to(B16)
    assert torch.equal(xb.float(), x32)
    val = ints((E,), g, 1, 3)
    geo = {F32: gc.typed_geometry(F, 4), B16: gc.typed_geometry(F, 2)}
    assert gc.pick_geometry(F) == geo[F32]
    assert gc.GCN_F32.get(F, geo[F32]) == geo[F32] and gc.GCN_BF16.get(F, geo[B16]) == geo[B16]
    print("F = %d: fp32 x (vec, group, ntiles) = %s, bf16 x = %s" % (F, geo[F32], geo[B16]))
    runs = 0
    for v in (val, None):
        agg = gnc.Aggregator_GCN(G.ptr, G.idx, v, F, F)
        agg.schedule_balanced(CHUNK)
        assert_row_classes(agg, ptr)
        total = {"sum": gcn_block(G, x32, v, 0, V, "sum"), "max": gcn_block(G, x32, v, 0, V, "max")}
        total["mean"] = total["sum"]
        assert float(total["sum"].abs().max()) < 2 ** 24
        for reduce in ("sum", "mean", "max"):
            for relu in (False, True):
                what = "F %d val %s %s relu %d" % (F, v is not None, reduce, relu)
                ys = {}
                for x in (x32, xb):
                    for ydt in (F32, B16):
                        y = poisoned((V, F), ydt)
                        aligned(x, y)
                        agg.run(x, y, 512, "balanced", reduce=reduce, relu=relu)
                        assert torch.equal(y, gcn_want(total[reduce], G.deg, reduce, relu, ydt)), "%s, balanced, x %s y %s" % (what, x.dtype, ydt)
                        ys[x.dtype, ydt] = y
                        runs += 1
                for xdt in (F32, B16):
                    assert torch.equal(ys[xdt, B16], ys[xdt, F32].to(B16)), what   # the fp32 y of the same call, rounded once
                # rows mode, the canonical CSR-order chains: fp32 only (the typed call refuses GNNAGG_MODE_ROWS unless "fast_rows" turns it
                # into the balanced order run above)
                y = poisoned((V, F))
                agg.run(x32, y, 512, 0, reduce=reduce, relu=relu)
                assert torch.equal(y, gcn_want(total[reduce], G.deg, reduce, relu, F32)), "%s, rows" % what
                runs += 1
    print("F = %d: %d runs equal to the float64 gather-and-reduce" % (F, runs))


@pytest.mark.parametrize("F", GCN_FEATS)
def test_gcn_with_nn_typed_against_run_and_matmul(F):
    """y as run() writes it on the same handle, transformed the product of y AS STORED (check_product); which entries take the epilogue
    depends on more than the geometry (geometry_census.py), so last_nn_path is printed, not asserted"""
    OUT = 8
    ptr, idx = census_graph()
    G = Graph(ptr, idx, len(ptr) - 1)
    V, E = G.V, G.E
    g = gen(200 + F)
    x32, w32, val = ints((V, F), g), ints((F, OUT), g, -2, 2), ints((E,), g, 1, 3)
    agg = gnc.Aggregator_GCN(G.ptr, G.idx, val, F, OUT)
    agg.schedule_balanced(CHUNK)
    assert_row_classes(agg, ptr)
    paths = []
    for xdt in (F32, B16):
        x = x32.to(xdt)
        for relu in (False, True):
            t_f32 = None
            for ydt, wdt, tdt in PRODUCTS:
                tag = "F %d -> %d, x %s y %s t %s relu %d" % (F, OUT, xdt, ydt, tdt, relu)
                w = w32.to(wdt)
                y, t = poisoned((V, F), ydt), poisoned((V, OUT), tdt)
                aligned(x, y, w, t)
                agg.run_with_nn_typed(x, y, w, t, "balanced", "sum", relu)
                paths.append(agg.last_nn_path())
                y2 = poisoned((V, F), ydt)
                agg.run(x, y2, 512, "balanced", relu=relu)
                assert torch.equal(y, y2), tag
                check_product(y, w, t, t_f32, what=tag)
                if ydt == B16 and tdt == F32:
                    t_f32 = t
    print("F = %d: geometry fp32 x %s, bf16 x %s; last_nn_path per call (1 = epilogue, 2 = GEMM behind): %s"
          % (F, gc.typed_geometry(F, 4), gc.typed_geometry(F, 2), paths))
    assert set(paths) <= {1, 2}


def split_rows(agg, V):
    """a restated locality schedule is in force and cuts rows into several items (scratch slots, the ordered combine)"""
    _, _, tg = agg.get_schedule("scheduled")
    assert len(tg) > V >= len(np.unique(tg))
    return len(tg)


@pytest.mark.parametrize("F", sorted(gc.GCN_F32))
def test_gcn_item_kernels_and_combine_every_geometry(F):
    """the item kernels (one work item per lane group on a work list) and k_combine, which the balanced and rows modes above leave to the
    plan kernels: scheduled mode on a locality schedule in the restated order ("fast_scheduled" = 0), fp32 only"""
    ptr, idx = census_graph()
    G = Graph(ptr, idx, len(ptr) - 1)
    V, E = G.V, G.E
    g = gen(250 + F)
    x32, val = ints((V, F), g), ints((E,), g, 1, 3)
    print("F = %d: (vec, group, ntiles) = %s" % (F, gc.GCN_F32[F]))
    for v in (val, None):
        agg = gnc.Aggregator_GCN(G.ptr, G.idx, v, F, F)
        agg.set_option("fast_scheduled", 0)
        agg.schedule(gnc.Schedule.locality, [3])
        split_rows(agg, V)
        total = {"sum": gcn_block(G, x32, v, 0, V, "sum"), "max": gcn_block(G, x32, v, 0, V, "max")}
        total["mean"] = total["sum"]
        for reduce in ("sum", "mean", "max"):
            for relu in (False, True):
                y = poisoned((V, F))
                aligned(x32, y)
                agg.run(x32, y, 512, 1, reduce=reduce, relu=relu)
                assert torch.equal(y, gcn_want(total[reduce], G.deg, reduce, relu, F32)), "F %d val %s %s relu %d" % (F, v is not None, reduce, relu)


# ------------------------------------------------------------------------------------------------------------ 2. GAT
GAT_SHAPES =sorted(set(gc.GAT_F32) | set(gc.GAT_BF16))


def newval_ref(ptr, idx, att, H, slope=0.2):
    """exp(leaky(att[r, h, 0] + att[j, h, 1])) per edge and head: the fp32 logit the kernels form, exponentiated in float64"""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    s = att[rows, :, 0] + att[idx, :, 1]            # fp32, one rounding, as in edge_weight()
    l = s * np.float32(slope)
    return np.exp(np.where(s > l, s, l).astype(np.float64))


def judge_gat(y, ref, scale, what):
    """assert_within of tests/test_gpu_bf16_gat.py, the worst ratio against its bound printed first"""
    y = y.cpu().numpy()
    err = np.abs(y.astype(np.float64) - ref.astype(np.float64))
    print("%s: worst |y - ref| / bound = %.4f" % (what, float((err / (1e-5 * scale.astype(np.float64) + 1e-30)).max())))
    assert_within(y, ref, scale, what)


@pytest.mark.parametrize("H,D", GAT_SHAPES)
def test_gat_every_geometry_meets_the_oracle_bound(H, D):
    ptr, idx = census_graph()
    V, E, F = len(ptr) - 1, len(idx), H * D
    geo = {F32: gc.typed_geometry(F, 4, D), B16: gc.typed_geometry(F, 2, D)}
    assert gc.pick_geometry(F, D) == geo[F32]
    assert gc.GAT_F32.get((H, D), geo[F32]) == geo[F32] and gc.GAT_BF16.get((H, D), geo[B16]) == geo[B16]
    print("%d x %d: fp32 x (vec, group, ntiles) = %s, bf16 x = %s" % (H, D, geo[F32], geo[B16]))
    att = rand((V, H, 2), 300 + F + H)
    xb, x32 = bf16_x(V, F, 400 + F + H)
    dx32, datt = dev(x32), dev(att)
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    agg.schedule_balanced(CHUNK)
    assert_row_classes(agg, ptr)
    ref = orc.gat_fused(ptr, idx, att, x32, H)
    scale = gat_scale(ptr, idx, att, x32, H) + np.abs(ref)
    nv_ref = newval_ref(ptr, idx, att, H)
    # balanced, with newval: the fp32 run against the oracle, the other three dtype pairs against it bit for bit
    y32, nv32 = full((V, F)), full((E, H))
    aligned(dx32, xb, datt, y32, nv32)
    agg.run(dx32, datt, y32, 128, "balanced", heads=H, newval=nv32)
    judge_gat(y32, ref, scale, "%d x %d balanced" % (H, D))
    np.testing.assert_allclose(nv32.cpu().numpy(), nv_ref, rtol=1e-6)   # (the bar of tests/test_gpu_parity.py)
    for x in (dx32, xb):
        for ydt in (F32, B16):
            y, nv = full((V, F), ydt), full((E, H))
            aligned(y, nv)
            agg.run(x, datt, y, 128, "balanced", heads=H, newval=nv)
            assert torch.equal(y, y32.to(ydt)) and torch.equal(nv, nv32), "%d x %d balanced, x %s y %s" % (H, D, x.dtype, ydt)
            y.fill_(7.0)
            agg.run(x, datt, y, 128, "balanced", heads=H)
            assert torch.equal(y, y32.to(ydt)), "%d x %d balanced without newval, x %s y %s" % (H, D, x.dtype, ydt)
    # the max-shifted softmax: the same judge (mild logits), the same exactness between the dtype pairs
    ys = full((V, F))
    agg.run(dx32, datt, ys, 128, "balanced", heads=H, stable=True)
    judge_gat(ys, ref, scale, "%d x %d stable" % (H, D))
    for x in (dx32, xb):
        for ydt in (F32, B16):
            y = full((V, F), ydt)
            agg.run(x, datt, y, 128, "balanced", heads=H, stable=True)
            assert torch.equal(y, ys.to(ydt)), "%d x %d stable, x %s y %s" % (H, D, x.dtype, ydt)
    # rows mode (fp32 only): the rows plan (hub rows on the long-row kernel where D % 32 == 0), and with newval the item kernels
    yr, nvr = full((V, F)), full((E, H))
    agg.run(dx32, datt, yr, 128, 0, heads=H)
    judge_gat(yr, ref, scale, "%d x %d rows" % (H, D))
    yr.fill_(7.0)
    agg.run(dx32, datt, yr, 128, 0, heads=H, newval=nvr)
    judge_gat(yr, ref, scale, "%d x %d rows with newval" % (H, D))
    np.testing.assert_allclose(nvr.cpu().numpy(), nv_ref, rtol=1e-6)


@pytest.mark.parametrize("H,D", sorted(gc.GAT_F32))
def test_gat_item_kernels_and_combine_every_geometry(H, D):
    """k_gat_items on a work list and the GAT k_combine (see the GCN test of the same name): a restated locality schedule, fp32 only"""
    ptr, idx = census_graph()
    V, F = len(ptr) - 1, H * D
    print("%d x %d: (vec, group, ntiles) = %s" % (H, D, gc.GAT_F32[(H, D)]))
    att = rand((V, H, 2), 300 + F + H)
    _, x32 = bf16_x(V, F, 400 + F + H)
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    agg.set_option("fast_scheduled", 0)
    agg.schedule(gnc.Schedule.locality, [3])
    split_rows(agg, V)
    dx32, datt, y = dev(x32), dev(att), full((V, F))
    aligned(dx32, datt, y)
    agg.run(dx32, datt, y, 128, 1, heads=H)
    ref = orc.gat_fused(ptr, idx, att, x32, H)
    judge_gat(y, ref, gat_scale(ptr, idx, att, x32, H) + np.abs(ref), "%d x %d items" % (H, D))


# ------------------------------------------------------------------------------------------------------------ 3. gnnagg_pack_rows
@pytest.mark.parametrize("F", sorted(gc.GCN_F32))
def test_pack_rows_every_geometry(F):
    n_src = 300
    x = dev(rand((n_src, F), 500 + F))
    rng = np.random.default_rng(F)
    ids_h = np.concatenate([rng.permutation(n_src), rng.integers(0, n_src, 157), [0, 0, n_src - 1, n_src - 1]]).astype(np.int32)
    ids = dev(ids_h)
    out = poisoned((len(ids_h), F))
    aligned(x, ids, out)
    print("F = %d: (vec, group, ntiles) = %s" % (F, gc.GCN_F32[F]))
    _lib.check(gnc.lib().gnnagg_pack_rows(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(ids.data_ptr()), len(ids_h), F,
                                          ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(out, x[ids.long()])


# ------------------------------------------------------------------------------------------------------------ 4. run_v2, run_dot
_TGRAPH = []


def attention_graph():
    """threshold_graph of tests/test_gpu_gatv2.py with few source rows beyond V (a 1024-column case stays small), its row classes asserted"""
    if not _TGRAPH:
        ptr, idx, n_src = threshold_graph(n_src_extra=300)
        deg = np.diff(ptr)
        V = len(ptr) - 1
        assert V % 8 != 0 and V % 4 != 0 and idx.max() == n_src - 1
        for n in (0, 1, BATCH - 1, BATCH, BATCH + 1, 2 * THRESHOLDS[-1], 2 * THRESHOLDS[-1] + 1, 3 * THRESHOLDS[-1] + 37):
            assert (deg == n).any()
        for t in THRESHOLDS:
            assert (deg == t - 1).any() and (deg == t).any() and (deg == t + 1).any()
        assert ((deg[1:-1] == 0) & (deg[:-2] > 0) & (deg[2:] > 0)).any()   # an empty row between two others
        assert ((deg > THRESHOLDS[-2]) & (deg <= THRESHOLDS[-1])).any()      # a long row of one segment (stored directly)
        assert (deg > 2 * THRESHOLDS[-1]).any()                              # rows of 2, 3 and more segments: scratch slots and the merge
        _TGRAPH.append((ptr, idx, n_src))
    return _TGRAPH[0]


def print_attention_geometry(H, D):
    per = gc.GATV2[(H, D)]
    for esize, name in ((4, "fp32"), (2, "bf16")):
        assert gc.gatv2_geometry(H * D, H, esize) == per[esize]
        print("%d x %d %s x: (segred, vec, group, nf_raw, nf, lph) = %s" % (H, D, name, per[esize]))


def offset_view(x, lead, dt):
    """x's values at an element offset of `lead` into a buffer of its own: (buffer, view)"""
    n = x.numel()
    buf = torch.zeros(n + lead + 3, device=DEV, dtype=dt)
    view = buf[lead:lead + n].view(x.shape)
    view.copy_(x)
    return buf, view


@pytest.mark.parametrize("H,D", sorted(gc.GATV2))
def test_run_v2_every_geometry(H, D):
    ptr, idx, n_src = attention_graph()
    V, F = len(ptr) - 1, H * D
    print_attention_geometry(H, D)
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    ps, pd, a = bf16_pair((n_src, F), 600 + F + H), bf16_pair((V, F), 700 + F + H), att_vec(H, D, 800 + F)
    aligned(ps[0], ps[1], pd[0], pd[1])
    judge_v2(agg, ptr, idx, ps, pd, a, H, "census %dx%d" % (H, D))
    # unaligned views (an element offset of 1: x_aligned = 0, element-wise loads and stores on the same instantiation): the same bits
    da = dev(a)
    for i, dt in ((1, F32), (0, B16)):
        (bs, vs), (bd, vd) = offset_view(ps[i], 1, dt), offset_view(pd[i], 1, dt)
        keep_s, keep_d = bs.clone(), bd.clone()
        for ydt in (F32, B16):
            y = full((V, F), ydt)
            aligned(y, da)
            agg.run_v2(ps[i], pd[i], da, y, heads=H)
            by = full((V * F + 4,), ydt)
            vy = by[1:1 + V * F].view(V, F)
            assert all(t.data_ptr() % 16 != 0 for t in (vs, vd, vy))
            agg.run_v2(vs, vd, da, vy, heads=H)
            assert torch.equal(vy, y), "%d x %d: unaligned views differ from the aligned run (%s x, %s y)" % (H, D, dt, ydt)
            assert (by[:1] == 7.0).all() and (by[1 + V * F:] == 7.0).all()
        assert torch.equal(bs, keep_s) and torch.equal(bd, keep_d)


@pytest.mark.parametrize("H,D", sorted(gc.GATV2))
def test_run_dot_every_geometry(H, D):
    ptr, idx, n_src = attention_graph()
    V, F = len(ptr) - 1, H * D
    print_attention_geometry(H, D)
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    pq, pk, pv = bf16_pair((V, F), 900 + F + H), bf16_pair((n_src, F), 1000 + F + H), bf16_pair((n_src, F), 1100 + F + H)
    aligned(pq[0], pq[1], pk[0], pk[1], pv[0], pv[1])
    judge_dot(agg, ptr, idx, pq, pk, pv, H, "census %dx%d" % (H, D))
    # unaligned, pitched views (pitched of tests/test_gpu_dot_attn.py): the same bits
    for i, dt in ((1, F32), (0, B16)):
        es = pq[i].element_size()
        (bq, vq), (bk, vk), (bv, vv) = pitched(pq[i], F + 3, 1, dt), pitched(pk[i], F + 1, 3, dt), pitched(pv[i], F + 1, 5, dt)
        keep = [b.clone() for b in (bq, bk, bv)]
        for ydt in (F32, B16):
            y = full((V, F), ydt)
            aligned(y)
            agg.run_dot(pq[i], pk[i], pv[i], y, heads=H)
            by = full((V * F + 4,), ydt)
            vy = by[1:1 + V * F].view(V, F)
            assert all(t.data_ptr() % 16 != 0 for t in (vq, vk, vv, vy))
            assert (vq.stride(0) * es) % 16 != 0 or (vk.stride(0) * es) % 16 != 0
            agg.run_dot(vq, vk, vv, vy, heads=H)
            assert torch.equal(vy, y), "%d x %d: unaligned views differ from the aligned run (%s x, %s y)" % (H, D, dt, ydt)
            assert (by[:1] == 7.0).all() and (by[1 + V * F:] == 7.0).all()
        assert all(torch.equal(b, c) for b, c in zip((bq, bk, bv), keep))


def linear_ref(ptr, idx, xs, xd, a, H):
    """float64 GATv2 with the leaky function REMOVED (slope 1: the score is linear): e_j = sum_c a[h, c] (xd[r] + xs[j])"""
    V, F = len(ptr) - 1, xs.shape[1]
    D = F // H
    xs64, xd64, a64 = xs.astype(np.float64), xd.astype(np.float64), a.astype(np.float64).reshape(1, H, D)
    y = np.zeros((V, F))
    for r in range(V):
        j = idx[ptr[r]:ptr[r + 1]]
        if len(j) == 0:
            continue
        z = (xd64[r][None, :] + xs64[j]).reshape(len(j), H, D)
        e = (a64 * z).sum(axis=2)
        w = np.exp(e - e.max(axis=0, keepdims=True))
        w /= w.sum(axis=0, keepdims=True)
        y[r] = (np.repeat(w, D, axis=1) * xs64[j]).sum(axis=0)
    return y


@pytest.mark.parametrize("slope", [0.0, 1.0])
@pytest.mark.parametrize("H,D", [(3, 16), (1, 150)])   # segmented in both types (3 heads in a 16- / 8-lane group); general, 3 -> 4 fragments
def test_run_v2_at_the_two_allowed_end_points_of_the_slope(H, D, slope):
    ptr, idx, n_src = attention_graph()
    V, F = len(ptr) - 1, H * D
    per = gc.GATV2[(H, D)]
    assert per[4][0] == per[2][0] == (D == 16)
    print_attention_geometry(H, D)
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    ps, pd, a = bf16_pair((n_src, F), 1200 + F), bf16_pair((V, F), 1300 + F), att_vec(H, D, 1400 + F)
    y, ref, bound = judge_v2(agg, ptr, idx, ps, pd, a, H, "slope %g %dx%d" % (slope, H, D), slope=slope)
    if slope == 1.0:
        # the judge itself: at slope 1 the leaky function is the identity (the margin of test_equal_scores_give_the_plain_mean)
        lin = linear_ref(ptr, idx, ps[2], pd[2], a, H)
        assert (np.abs(ref - lin) <= 1e-7 * bound).all()
    else:
        # slope 0 is a ReLU inside the score: it does change the result (the case is not the linear one in disguise)
        other, _, _ = gatv2_ref(ptr, idx, ps[2], pd[2], a, H, 1.0, block_edges=judge_block(F))
        assert (np.abs(ref - other) > bound).any()
