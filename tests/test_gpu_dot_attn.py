"""GPU: scaled dot-product attention over the edges -- gnnagg_dot_attn_run (Aggregator_GAT.run_dot): edge score scale * q[i] . k[j] per head,
online max-shifted edge softmax and the weighted sum of the gathered v rows in one kernel (csrc/agg_dot.hip).

The judge is the float64 restatement in tests/test_dot_attn_host.py.  An fp32 y is held to the project's 1e-5 bar widened by the score's own
condition number,
    |y - ref|[r, hD + c] <= 1e-5 * (1 + L[r, h]) * S[r, hD + c],   L = max_j |scale| sum_c |q k|,   S = sum_j alpha_j |v[j]|,
over the WHOLE output (y is pre-filled with 7.0; rows without edges must be exactly +0); a bf16 y must be bit-equal to one rounding of the
fp32-y run on the same inputs.  bf16 inputs are judged on their exact widening -- the fp32 input of a case IS that widening, so one
reference serves the four dtype pairs.  Every case prints its worst ratio against the bound."""
import ctypes
import math

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_dot_attn_host import dot_attn_bound, dot_attn_ref
from test_gatv2_host import gatv2_ref, worst_ratio
from test_gpu_bf16_gat import DEV, GRAPHS, HD, dev
from test_gpu_gatv2 import att_vec, bf16_pair, full, judge_block, threshold_graph

pytestmark = pytest.mark.gpu

F32, B16 = torch.float32, torch.bfloat16
THRESHOLDS = gnc.Aggregator_GAT.GATV2_THRESHOLDS
BATCH = THRESHOLDS[0]


def f32_scale(scale, D):
    """the fp32 value the kernel gets"""
    return np.float32(1.0 / math.sqrt(D) if scale is None else scale)


def run_pairs_and_judge(agg, ptr, idx, pq, pk, pv, H, what, scale=None):
    """the four dtype pairs on one set of values; returns (fp32-in fp32-out y as numpy, reference, bound, S)"""
    V, F = len(ptr) - 1, pk[2].shape[1]
    ref, L, S = dot_attn_ref(ptr, idx, pq[2], pk[2], pv[2], H, f32_scale(scale, F // H), block_edges=judge_block(F))
    bound = dot_attn_bound(L, S, H)
    empty = np.diff(ptr) == 0
    out = None
    for i, tag in ((1, "fp32 x"), (0, "bf16 x")):
        q, k, v = pq[i], pk[i], pv[i]
        y32, y16 = full((V, F)), full((V, F), B16)
        agg.run_dot(q, k, v, y32, heads=H, scale=scale)
        agg.run_dot(q, k, v, y16, heads=H, scale=scale)
        y = y32.cpu().numpy()
        ratio = worst_ratio(y, ref, bound)
        print("%s, %s: worst |y - ref| / bound = %.4f" % (what, tag, ratio))
        assert np.isfinite(y).all(), "%s, %s: non-finite output" % (what, tag)
        assert ratio <= 1.0, "%s, %s -> fp32 y: worst ratio %.3g against the bound" % (what, tag, ratio)
        assert np.all(y[empty] == 0) and not np.signbit(y[empty]).any()
        assert torch.equal(y16, y32.to(B16)), "%s, %s: the bf16 y is not one rounding of the fp32 y" % (what, tag)
        if out is None:
            out = y
    return out, ref, bound, S


# ------------------------------------------------------------------------------------------ 1. the project's graphs, every head shape
@pytest.mark.parametrize("graph", ["uniform", "powerlaw"])
@pytest.mark.parametrize("H,D", HD)
def test_graphs_head_shapes_and_dtype_pairs(graph, H, D):
    ptr, idx = GRAPHS[graph]()
    V, F = len(ptr) - 1, H * D
    deg = np.diff(ptr)
    if graph == "uniform":
        assert (deg == 0).any()
    else:
        assert deg.max() > 2 * THRESHOLDS[-1]   # hub rows: several segments and the ordered merge
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    run_pairs_and_judge(agg, ptr, idx, bf16_pair((V, F), 1000 + F + H), bf16_pair((V, F), 2000 + F + H), bf16_pair((V, F), 3000 + F + H), H,
                        "%s %dx%d" % (graph, H, D))


# ------------------------------------------------------------------------------------------ 1b. two and four fragments per lane
# HD stops at 8 x 32 and the general geometry's 10 fragments: (4, 128) is 2 fragments in fp32, (8, 128) 4 in fp32 and 2 in bf16, (1, 100) and
# (1, 200) the general geometry's 2 and 4 -- the geometries whose batch is 2 edges instead of 4 (csrc/agg_dot.hip: dot_batch)
@pytest.mark.parametrize("H,D", [(4, 128), (8, 128), (1, 100), (1, 200)])
def test_wide_rows_of_two_and_four_fragments_per_lane(H, D):
    ptr, idx = GRAPHS["powerlaw"]()
    V, F = len(ptr) - 1, H * D
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    run_pairs_and_judge(agg, ptr, idx, bf16_pair((V, F), 1100 + F), bf16_pair((V, F), 2100 + F), bf16_pair((V, F), 3100 + F), H,
                        "powerlaw %dx%d" % (H, D))


# ------------------------------------------------------------------------------------------ 2. every row length where the walk changes
@pytest.mark.parametrize("H,D", [(1, 3), (1, 8), (4, 8), (8, 16), (1, 128), (8, 32), (1, 602), (2, 301)])
def test_row_lengths_at_every_threshold_and_packed_views(H, D):
    ptr, idx, n_src = threshold_graph()
    V, F = len(ptr) - 1, H * D
    deg = np.diff(ptr)
    assert V % 8 != 0 and V % 4 != 0 and idx.max() == n_src - 1 and n_src > 10 * V
    for n in (0, 1, BATCH - 1, BATCH, BATCH + 1, 2 * THRESHOLDS[-1], 2 * THRESHOLDS[-1] + 1, 3 * THRESHOLDS[-1] + 37):
        assert (deg == n).any()
    for t in THRESHOLDS:
        assert (deg == t - 1).any() and (deg == t).any() and (deg == t + 1).any()
    assert ((deg[1:-1] == 0) & (deg[:-2] > 0) & (deg[2:] > 0)).any()   # an empty row between two others
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    pq, pk, pv = bf16_pair((n_src, F), 4 + F), bf16_pair((n_src, F), 5 + F), bf16_pair((n_src, F), 6 + F)
    run_pairs_and_judge(agg, ptr, idx, pq, pk, pv, H, "thresholds %dx%d" % (H, D))
    # the column views of one [n_src, 3F] tensor against three contiguous tensors: the same bits
    for i, dt in ((1, F32), (0, B16)):
        packed = torch.cat([pq[i], pk[i], pv[i]], dim=1)
        q, k, v = packed[:, :F], packed[:, F:2 * F], packed[:, 2 * F:]
        assert q.stride(0) == 3 * F and not k.is_contiguous() and k.data_ptr() == packed.data_ptr() + F * packed.element_size()
        for ydt in (F32, B16):
            y_views, y_dense = full((V, F), ydt), full((V, F), ydt)
            agg.run_dot(q, k, v, y_views, heads=H)
            agg.run_dot(pq[i], pk[i], pv[i], y_dense, heads=H)
            assert torch.equal(y_views, y_dense), "packed views differ from contiguous operands (%s x, %s y)" % (dt, ydt)


# ------------------------------------------------------------------------------------------ 3. where the maximum sits
def scores(ptr, idx, q, k, H, scale):
    """float64 scores [E, H] (small graphs)"""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    t = q.astype(np.float64)[rows] * k.astype(np.float64)[idx]
    return float(np.float32(scale)) * t.reshape(len(idx), H, -1).sum(axis=2)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("H,D", [(1, 8), (4, 3)])
def test_the_row_maximum_on_the_first_a_middle_and_the_last_edge(where, H, D):
    """the rescale fires never after the first batch (maximum first), on the way (middle), or with the very last edge"""
    ptr, idx, n_src = threshold_graph(n_src_extra=300)
    V, F = len(ptr) - 1, H * D
    deg = np.diff(ptr)
    g = torch.Generator().manual_seed(11)
    qb = (torch.randn((V, F), generator=g).abs() + 0.5).to(B16)
    pq = (qb.to(DEV), qb.float().to(DEV), qb.float().numpy())
    _, _, k_np = bf16_pair((n_src, F), 12)
    special = n_src - 1
    k_np[special] = 8.0           # q > 0 and a large positive row: by far the largest score of any row it appears in
    pk = (dev(k_np).to(B16), dev(k_np), k_np)
    idx = np.where(idx == special, 0, idx).astype(np.int32)
    pos = {"first": ptr[:-1], "middle": ptr[:-1] + deg // 2, "last": ptr[1:] - 1}[where][deg > 0]
    idx[pos] = special
    e = scores(ptr, idx, pq[2], k_np, H, 1.0)
    for r, p in zip(np.flatnonzero(deg > 0), pos):
        assert (e[ptr[r]:ptr[r + 1]].argmax(axis=0) == p - ptr[r]).all()
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    run_pairs_and_judge(agg, ptr, idx, pq, pk, bf16_pair((n_src, F), 13), H, "maximum %s %dx%d" % (where, H, D), scale=1.0)


# ------------------------------------------------------------------------------------------ 4. scores beyond expf's range
@pytest.mark.parametrize("graph,H,D", [("uniform", 1, 128), ("powerlaw", 8, 16), ("uniform", 2, 301), ("powerlaw", 4, 3)])
def test_scores_beyond_88_stay_finite_and_within_the_bound(graph, H, D):
    ptr, idx = GRAPHS[graph]()
    V, F = len(ptr) - 1, H * D
    pq, pk, pv = bf16_pair((V, F), 21, 30.0), bf16_pair((V, F), 22, 30.0), bf16_pair((V, F), 23, 30.0)
    if graph == "uniform":
        e = scores(ptr, idx, pq[2], pk[2], H, 1.0)
        assert e.max() > 88.0 and e.min() < -88.0   # an unshifted expf would give +inf and 0
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    y, _, _, _ = run_pairs_and_judge(agg, ptr, idx, pq, pk, pv, H, "inputs x30 %s %dx%d" % (graph, H, D), scale=1.0)
    assert np.isfinite(y).all()


# ------------------------------------------------------------------------------------------ 5. equal scores: the plain mean
@pytest.mark.parametrize("zero", ["q", "scale"])
@pytest.mark.parametrize("H,D", [(1, 8), (4, 3), (1, 128)])
def test_equal_scores_give_the_plain_mean(zero, H, D):
    ptr, idx = GRAPHS["uniform"]()
    V, F = len(ptr) - 1, H * D
    pq, pk, pv = bf16_pair((V, F), 31), bf16_pair((V, F), 32), bf16_pair((V, F), 33)
    if zero == "q":
        pq = (torch.zeros((V, F), device=DEV, dtype=B16), torch.zeros((V, F), device=DEV), np.zeros((V, F), np.float32))
    scale = 0.0 if zero == "scale" else None
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    y, ref, bound, S = run_pairs_and_judge(agg, ptr, idx, pq, pk, pv, H, "%s = 0, %dx%d" % (zero, H, D), scale=scale)
    deg = np.diff(ptr)
    mean = np.zeros((V, F))
    np.add.at(mean, np.repeat(np.arange(V), deg), pv[2].astype(np.float64)[idx])
    mean[deg > 0] /= deg[deg > 0, None]
    assert np.array_equal(bound, 1e-5 * S)         # L = 0: the plain 1e-5 bar
    assert (np.abs(ref - mean) <= 1e-7 * bound).all()   # the judge itself: the mean to 1e-12 of sum |v| / n
    assert worst_ratio(y, mean, 1e-5 * S) <= 1.0


# ------------------------------------------------------------------------------------------ 6. the scale
@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (2, 301), (4, 3)])
@pytest.mark.parametrize("dt", [F32, B16])
def test_default_power_of_two_and_negative_scale(H, D, dt):
    ptr, idx = GRAPHS["powerlaw"]()
    V, F = len(ptr) - 1, H * D
    pq, pk, pv = bf16_pair((V, F), 71), bf16_pair((V, F), 72), bf16_pair((V, F), 73)
    i = 0 if dt == B16 else 1
    q, k, v = pq[i], pk[i], pv[i]
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    y_none, y_expl = full((V, F), dt), full((V, F), dt)
    agg.run_dot(q, k, v, y_none, heads=H)
    agg.run_dot(q, k, v, y_expl, heads=H, scale=1.0 / math.sqrt(D))
    assert torch.equal(y_none, y_expl)
    # a power of two commutes with every rounding: scaling q beforehand (exact, in bf16 too) gives the same bits
    y_in, y_pre = full((V, F), dt), full((V, F), dt)
    agg.run_dot(q, k, v, y_in, heads=H, scale=0.25)
    q4 = q * 0.25
    assert torch.equal(q4.double(), q.double() * 0.25)
    agg.run_dot(q4, k, v, y_pre, heads=H, scale=1.0)
    assert torch.equal(y_in, y_pre)
    if dt == F32:
        run_pairs_and_judge(agg, ptr, idx, pq, pk, pv, H, "scale -0.7 %dx%d" % (H, D), scale=-0.7)


# ------------------------------------------------------------------------------------------ 7. aliasing, repeatability, alignment
def pitched(x, pitch, lead, dt):
    """x's values in a buffer whose rows are `pitch` elements apart and start `lead` elements in: (buffer, the [rows, F] view)"""
    n, F = x.shape
    buf = torch.zeros(lead + n * pitch + 2, device=DEV, dtype=dt)
    view = buf[lead:lead + n * pitch].view(n, pitch)[:, :F]
    view.copy_(x)
    return buf, view


@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (2, 301)])
@pytest.mark.parametrize("dt", [F32, B16])
def test_shared_input_repeat_and_unaligned_views(H, D, dt):
    ptr, idx = GRAPHS["powerlaw"]()
    V, F = len(ptr) - 1, H * D
    assert idx.max() < V   # a square graph: one tensor can be q, k and v
    i = 0 if dt == B16 else 1
    x, k, v = bf16_pair((V, F), 41)[i], bf16_pair((V, F), 42)[i], bf16_pair((V, F), 43)[i]
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    y_shared, y_copy, y_again = full((V, F), dt), full((V, F), dt), full((V, F), dt)
    agg.run_dot(x, x, x, y_shared, heads=H)            # q, k and v: the same pointer
    agg.run_dot(x.clone(), x.clone(), x.clone(), y_copy, heads=H)
    agg.run_dot(x, x, x, y_again, heads=H)
    assert torch.equal(y_shared, y_copy) and torch.equal(y_shared, y_again)
    assert torch.isfinite(y_shared.float()).all()
    # the aligned dense run of three different operands ...
    y_dense = full((V, F), dt)
    agg.run_dot(x, k, v, y_dense, heads=H)
    # ... against views at odd element offsets with a pitch that is no multiple of 16 bytes: the same bits, inputs and the elements
    # around y untouched
    n = V * F
    es = x.element_size()
    (bq, vq), (bk, vk), (bv, vv) = pitched(x, F + 3, 1, dt), pitched(k, F + 1, 3, dt), pitched(v, F + 1, 5, dt)
    by = full((n + 4,), dt)
    vy = by[1:1 + n].view(V, F)
    assert vq.data_ptr() % 4 != 0 or dt == F32
    assert all(t.data_ptr() % 16 != 0 for t in (vq, vk, vv, vy))
    assert (vq.stride(0) * es) % 16 != 0 and (vk.stride(0) * es) % 16 != 0 and vk.stride(0) == vv.stride(0)
    keep = [b.clone() for b in (bq, bk, bv)]
    agg.run_dot(vq, vk, vv, vy, heads=H)
    assert torch.equal(vy, y_dense)
    assert all(torch.equal(b, c) for b, c in zip((bq, bk, bv), keep))
    assert (by[:1] == 7.0).all() and (by[1 + n:] == 7.0).all()
    # an aligned base with an unaligned pitch
    (_, vk2), (_, vv2) = pitched(k, F + 1, 0, dt), pitched(v, F + 1, 0, dt)
    y2 = full((V, F), dt)
    agg.run_dot(x, vk2, vv2, y2, heads=H)
    assert torch.equal(y2, y_dense)
    # the flat function is the same call
    y_flat = full((V, F), dt)
    gnc.dot_attn_run(agg, x, k, v, y_flat, heads=H)
    assert torch.equal(y_flat, y_dense)


# ------------------------------------------------------------------------------------------ 8. HIP graph
@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (2, 301)])
def test_graph_capture_and_replay(H, D):
    ptr, idx = GRAPHS["powerlaw"]()
    V, F = len(ptr) - 1, H * D
    qkv = torch.cat([bf16_pair((V, F), 51 + s)[0] for s in range(3)], dim=1)
    q, k, v = qkv[:, :F], qkv[:, F:2 * F], qkv[:, 2 * F:]
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    for ydt in (F32, B16):
        y = full((V, F), ydt)
        agg.run_dot(q, k, v, y, heads=H)       # warm call: the list of long rows, the scratch
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):              # (captures on a side stream: the call may neither allocate nor synchronise)
            agg.run_dot(q, k, v, y, heads=H)
        for seed in (55, 56):
            q.copy_(bf16_pair((V, F), seed)[0])
            y.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            eager = full((V, F), ydt)
            agg.run_dot(q, k, v, eager, heads=H)
            assert torch.equal(y, eager) and torch.isfinite(y.float()).all()


# ------------------------------------------------------------------------------------------ 9. one handle, both attention calls
def test_a_handle_serving_run_v2_and_run_dot_alternately():
    """the segment plan is built by whichever call comes first and the scratch grows for whichever needs more: call by call the bits of
    a fresh single-purpose handle"""
    ptr, idx = GRAPHS["powerlaw"]()
    V = len(ptr) - 1
    assert np.diff(ptr).max() > 2 * THRESHOLDS[-1]   # rows of several segments: the scratch is in use
    dptr, didx = dev(ptr), dev(idx)
    # (call, H, D, x dtype, y dtype): small F, large F, small F; the dtype and the kind change with it
    calls = [("dot", 4, 8, B16, F32), ("v2", 1, 8, F32, F32), ("dot", 1, 602, F32, B16), ("v2", 8, 16, B16, B16), ("dot", 1, 3, F32, F32),
             ("v2", 2, 301, F32, F32), ("dot", 8, 32, F32, F32), ("dot", 4, 8, B16, F32), ("v2", 1, 8, F32, F32)]

    def one(agg, kind, H, D, xdt, ydt, seed):
        F = H * D
        i = 0 if xdt == B16 else 1
        y = full((V, F), ydt)
        if kind == "dot":
            agg.run_dot(bf16_pair((V, F), seed)[i], bf16_pair((V, F), seed + 1)[i], bf16_pair((V, F), seed + 2)[i], y, heads=H)
        else:
            agg.run_v2(bf16_pair((V, F), seed)[i], bf16_pair((V, F), seed + 1)[i], dev(att_vec(H, D, seed + 2)), y, heads=H)
        return y
    for first in (0, 1):   # the plan built by a run_dot, and by a run_v2
        shared = gnc.Aggregator_GAT(dptr, didx, 8, 8)
        for n, (kind, H, D, xdt, ydt) in enumerate(calls[first:]):
            got = one(shared, kind, H, D, xdt, ydt, 90 + n)
            want = one(gnc.Aggregator_GAT(dptr, didx, H * D, H * D), kind, H, D, xdt, ydt, 90 + n)
            assert torch.equal(got, want), "call %d (%s %dx%d) on the shared handle differs from a fresh one" % (n, kind, H, D)
            assert torch.isfinite(got.float()).all()
    # and GATv2 on such a handle is still GATv2: the judge of its own tests
    H, D = 8, 16
    ps, pd, a = bf16_pair((V, H * D), 97), bf16_pair((V, H * D), 98), att_vec(H, D, 99)
    y = full((V, H * D))
    shared.run_v2(ps[1], pd[1], dev(a), y, heads=H)
    ref, L, S = gatv2_ref(ptr, idx, ps[2], pd[2], a, H, block_edges=judge_block(H * D))
    assert worst_ratio(y.cpu().numpy(), ref, 1e-5 * (1.0 + np.repeat(L, D, axis=1)) * S) <= 1.0


# ------------------------------------------------------------------------------------------ 10. refusals of the C-ABI
def test_cabi_refusals_leave_y_alone():
    ptr, idx = GRAPHS["uniform"]()
    V, F = len(ptr) - 1, 16
    dptr, didx = dev(ptr), dev(idx)
    gat = gnc.Aggregator_GAT(dptr, didx, F, F)
    gcn = gnc.Aggregator_GCN(dptr, didx, None, F, F)
    big = gnc.Aggregator_GAT.GATV2_MAX_FEAT + 8
    x, y = torch.zeros((V, big), device=DEV), full((V, big))
    L = gnc.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def refused(text, h=None, q=x, k=x, v=x, qp=big, kvp=big, xt=0, yv=y, yt=0, feat=F, heads=2, scale=0.5):
        rc = L.gnnagg_dot_attn_run(gat._h if h is None else h, None if q is None else p(q), qp, None if k is None else p(k),
                                   None if v is None else p(v), kvp, xt, None if yv is None else p(yv), yt, feat, heads, ctypes.c_float(scale))
        err = L.gnnagg_last_error()
        assert rc == _lib.ERR_ARG and b"gnnagg_dot_attn_run" in err and text in err, err
    refused(b"not a GAT aggregator", h=gcn._h)
    refused(b"d_q", q=None)
    refused(b"d_k", k=None)
    refused(b"d_v", v=None)
    refused(b"d_y", yv=None)
    refused(b"x_dtype 7", xt=7)
    refused(b"y_dtype -1", yt=-1)
    refused(b"feat = 0", feat=0)
    refused(b"feat = -4", feat=-4)
    refused(b"heads = 0", heads=0)
    refused(b"heads = 3", heads=3)
    refused(b"q_pitch = 15", qp=15)
    refused(b"kv_pitch = 15", kvp=15)
    refused(b"kv_pitch = -16", kvp=-16)
    refused(b"scale", scale=float("nan"))
    refused(b"scale", scale=float("inf"))
    refused(b"scale", scale=-float("inf"))
    refused(("limit of %d" % gnc.Aggregator_GAT.GATV2_MAX_FEAT).encode(), feat=big, heads=1)
    torch.cuda.synchronize()
    assert (y == 7.0).all()
    # the limit itself runs
    F = gnc.Aggregator_GAT.GATV2_MAX_FEAT
    pq, pk, pv = bf16_pair((V, F), 61, 0.5), bf16_pair((V, F), 62, 0.5), bf16_pair((V, F), 63)
    ok = full((V, F))
    gat.run_dot(pq[1], pk[1], pv[1], ok, heads=1)
    ref, Lc, S = dot_attn_ref(ptr, idx, pq[2], pk[2], pv[2], 1, f32_scale(None, F), block_edges=judge_block(F))
    ratio = worst_ratio(ok.cpu().numpy(), ref, dot_attn_bound(Lc, S, 1))
    print("F = %d: worst ratio %.4f" % (F, ratio))
    assert ratio <= 1.0
    with pytest.raises(gnc.GnnAggError, match="limit of"):
        gat.run_dot(x, x, x, y, heads=1)
