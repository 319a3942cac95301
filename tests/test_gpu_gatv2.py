"""GPU: GATv2 attention -- gnnagg_gatv2_run (Aggregator_GAT.run_v2): edge score a . leaky(xd[i] + xs[j]), online max-shifted edge softmax and
the weighted sum of the gathered rows in one kernel (csrc/agg_gatv2.hip).

The judge is the float64 restatement in tests/test_gatv2_host.py.  An fp32 y is held to the project's 1e-5 bar widened by the score's own
condition number,
    |y - ref|[r, hD + c] <= 1e-5 * (1 + L[r, h]) * S[r, hD + c],   L = max_j sum_c |a[h, c] l_jc|,   S = sum_j alpha_j |xs[j]|,
over the WHOLE output (y is pre-filled with 7.0; rows without edges must be exactly +0); a bf16 y must be bit-equal to one rounding of the
fp32-y run on the same inputs.  bf16 inputs are judged on their exact widening -- the fp32 input of a case IS that widening, so one
reference serves the four dtype pairs.  Every case prints its worst ratio against the bound."""
import ctypes

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib
from test_gatv2_host import gatv2_bound, gatv2_ref, worst_ratio
from test_gpu_bf16_gat import DEV, GRAPHS, HD, dev

pytestmark = pytest.mark.gpu

F32, B16 = torch.float32, torch.bfloat16
THRESHOLDS = gnc.Aggregator_GAT.GATV2_THRESHOLDS
BATCH = THRESHOLDS[0]


def bf16_pair(shape, seed, scale=1.0):
    """(bf16 device tensor, fp32 device tensor holding its exact widening, the widening as numpy)"""
    g = torch.Generator().manual_seed(seed)
    xb = (torch.randn(shape, generator=g) * scale).to(B16)
    return xb.to(DEV), xb.float().to(DEV), xb.float().numpy()


def att_vec(H, D, seed):
    return np.random.default_rng(seed).standard_normal((H, D), dtype=np.float32)


def full(shape, dtype=F32):
    return torch.full(shape, 7.0, device=DEV, dtype=dtype)


def judge_block(F):
    return max(256, (1 << 22) // F)   # edges per block of the float64 judge: ~32 MB per temporary


def run_pairs_and_judge(agg, ptr, idx, pair_s, pair_d, a, H, what, slope=0.2):
    """the four dtype pairs on one set of values; returns (fp32-in fp32-out y as numpy, reference, bound)"""
    (sb, s32, s_np), (db, d32, d_np) = pair_s, pair_d
    V, F = len(ptr) - 1, s_np.shape[1]
    da = dev(a)
    ref, L, S = gatv2_ref(ptr, idx, s_np, d_np, a, H, slope, block_edges=judge_block(F))
    bound = gatv2_bound(L, S, H)
    empty = np.diff(ptr) == 0
    out = None
    for xs, xd, tag in ((s32, d32, "fp32 x"), (sb, db, "bf16 x")):
        y32, y16 = full((V, F)), full((V, F), B16)
        agg.run_v2(xs, xd, da, y32, heads=H, slope=slope)
        agg.run_v2(xs, xd, da, y16, heads=H, slope=slope)
        y = y32.cpu().numpy()
        ratio = worst_ratio(y, ref, bound)
        print("%s, %s: worst |y - ref| / bound = %.4f" % (what, tag, ratio))
        assert np.isfinite(y).all(), "%s, %s: non-finite output" % (what, tag)
        assert ratio <= 1.0, "%s, %s -> fp32 y: worst ratio %.3g against the bound" % (what, tag, ratio)
        assert np.all(y[empty] == 0) and not np.signbit(y[empty]).any()
        assert torch.equal(y16, y32.to(B16)), "%s, %s: the bf16 y is not one rounding of the fp32 y" % (what, tag)
        if out is None:
            out = y
    return out, ref, bound


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
    pair = bf16_pair((V, F), 1000 + F + H)
    run_pairs_and_judge(agg, ptr, idx, pair, bf16_pair((V, F), 2000 + F + H), att_vec(H, D, F), H, "%s %dx%d" % (graph, H, D))


# ------------------------------------------------------------------------------------------ 2. every row length where the walk changes
def threshold_graph(n_src_extra=5000, seed=3):
    """rows of 0, 1, batch - 1, batch, batch + 1 edges, of every GATV2_THRESHOLDS value and its neighbours, of 2 and 3 segments and one of
    several more; an empty row between two others; V no multiple of the 4 or 8 rows of a workgroup; source ids far beyond V"""
    lens = [0, 1, BATCH - 1, BATCH, BATCH + 1, 2, 0, 7]
    for t in THRESHOLDS:
        lens += [t - 1, t, t + 1]
    seg = THRESHOLDS[-1]
    lens += [2 * seg - 1, 2 * seg, 2 * seg + 1, 0, 3 * seg + 37, 5]
    while len(lens) % 8 != 3:
        lens.append(len(lens) % 5)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    V = len(lens)
    n_src = V + n_src_extra
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_src, int(ptr[-1])).astype(np.int32)
    idx[rng.integers(0, len(idx), 50)] = n_src - 1
    idx[ptr[:-1][np.diff(ptr) > 0]] = rng.integers(V, n_src, int((np.diff(ptr) > 0).sum()))   # every row starts beyond V
    return ptr, idx, n_src


@pytest.mark.parametrize("H,D", [(1, 3), (1, 8), (4, 8), (8, 16), (1, 128), (8, 32), (1, 602), (2, 301)])
def test_row_lengths_at_every_threshold(H, D):
    ptr, idx, n_src = threshold_graph()
    V, F = len(ptr) - 1, H * D
    assert V % 8 != 0 and V % 4 != 0 and idx.max() == n_src - 1 and n_src > 10 * V
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    run_pairs_and_judge(agg, ptr, idx, bf16_pair((n_src, F), 5 + F), bf16_pair((V, F), 6 + F), att_vec(H, D, 7), H, "thresholds %dx%d" % (H, D))


# ------------------------------------------------------------------------------------------ 3. where the maximum sits
def scores(ptr, idx, xs, xd, a, H, slope=0.2):
    """float64 scores [E, H] (small graphs)"""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    z = xd.astype(np.float64)[rows] + xs.astype(np.float64)[idx]
    zs = z * float(np.float32(slope))
    return (a.astype(np.float64).reshape(1, -1) * np.where(z > zs, z, zs)).reshape(len(idx), H, -1).sum(axis=2)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("H,D", [(1, 8), (4, 3)])
def test_the_row_maximum_on_the_first_a_middle_and_the_last_edge(where, H, D):
    """the rescale fires never after the first batch (maximum first), on the way (middle), or with the very last edge"""
    ptr, idx, n_src = threshold_graph(n_src_extra=300)
    V, F = len(ptr) - 1, H * D
    deg = np.diff(ptr)
    a = np.abs(att_vec(H, D, 11)) + 0.5
    sb, s32, s_np = bf16_pair((n_src, F), 12)
    special = n_src - 1
    s_np[special] = 8.0           # a > 0 and a large positive row: by far the largest score of any row it appears in
    s32, sb = dev(s_np), dev(s_np).to(B16)
    idx = np.where(idx == special, 0, idx).astype(np.int32)
    pos = {"first": ptr[:-1], "middle": ptr[:-1] + deg // 2, "last": ptr[1:] - 1}[where][deg > 0]
    idx[pos] = special
    pair_d = bf16_pair((V, F), 13)
    e = scores(ptr, idx, s_np, pair_d[2], a, H)
    for r, p in zip(np.flatnonzero(deg > 0), pos):
        assert (e[ptr[r]:ptr[r + 1]].argmax(axis=0) == p - ptr[r]).all()
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    run_pairs_and_judge(agg, ptr, idx, (sb, s32, s_np), pair_d, a, H, "maximum %s %dx%d" % (where, H, D))


# ------------------------------------------------------------------------------------------ 4. scores beyond expf's range
@pytest.mark.parametrize("graph,H,D,scale", [("uniform", 1, 128, 30.0), ("powerlaw", 8, 16, 30.0), ("uniform", 2, 301, 8.0), ("powerlaw", 4, 3, 60.0)])
def test_scores_beyond_88_stay_finite_and_within_the_bound(graph, H, D, scale):
    ptr, idx = GRAPHS[graph]()
    V, F = len(ptr) - 1, H * D
    pair_s, pair_d = bf16_pair((V, F), 21, scale), bf16_pair((V, F), 22, scale)
    a = att_vec(H, D, 23)
    if graph == "uniform":
        e = scores(ptr, idx, pair_s[2], pair_d[2], a, H)
        assert e.max() > 88.0 and e.min() < -88.0   # an unshifted expf would give +inf and 0
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    y, ref, _ = run_pairs_and_judge(agg, ptr, idx, pair_s, pair_d, a, H, "scaled x%g %s %dx%d" % (scale, graph, H, D))
    assert np.isfinite(y).all()


# ------------------------------------------------------------------------------------------ 5. equal scores: the plain mean
@pytest.mark.parametrize("H,D", [(1, 8), (4, 3), (1, 128)])
def test_equal_scores_give_the_plain_mean(H, D):
    ptr, idx = GRAPHS["uniform"]()
    V, F = len(ptr) - 1, H * D
    pair_s, pair_d = bf16_pair((V, F), 31), bf16_pair((V, F), 32)
    a = np.zeros((H, D), np.float32)     # every score is 0
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    y, ref, bound = run_pairs_and_judge(agg, ptr, idx, pair_s, pair_d, a, H, "equal scores %dx%d" % (H, D))
    deg = np.diff(ptr)
    mean = np.zeros((V, F))
    np.add.at(mean, np.repeat(np.arange(V), deg), pair_s[2].astype(np.float64)[idx])
    mean[deg > 0] /= deg[deg > 0, None]
    assert (np.abs(ref - mean) <= 1e-7 * bound).all()   # the judge itself: the mean to 1e-12 of sum |x| / n (bound = 1e-5 * S here)
    assert worst_ratio(y, mean, bound) <= 1.0   # (L = 0: the plain 1e-5 bar)


# ------------------------------------------------------------------------------------------ 6. aliasing, repeatability, alignment
@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (2, 301)])
@pytest.mark.parametrize("dt", [F32, B16])
def test_shared_input_repeat_and_unaligned_views(H, D, dt):
    ptr, idx = GRAPHS["powerlaw"]()
    V, F = len(ptr) - 1, H * D
    xb, x32, _ = bf16_pair((V, F), 41)
    x = xb if dt == B16 else x32
    a = dev(att_vec(H, D, 42))
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    y_shared, y_copy, y_again = full((V, F), dt), full((V, F), dt), full((V, F), dt)
    agg.run_v2(x, x, a, y_shared, heads=H)            # xd is xs: the same pointer
    agg.run_v2(x, x.clone(), a, y_copy, heads=H)
    agg.run_v2(x, x, a, y_again, heads=H)
    assert torch.equal(y_shared, y_copy) and torch.equal(y_shared, y_again)
    assert torch.isfinite(y_shared.float()).all()
    # views at odd element offsets: the same bits, inputs and the elements around y untouched
    n = V * F
    bs, bd, by = torch.zeros(n + 3, device=DEV, dtype=dt), torch.zeros(n + 5, device=DEV, dtype=dt), full((n + 4,), dt)
    vs, vd, vy = bs[1:1 + n].view(V, F), bd[3:3 + n].view(V, F), by[1:1 + n].view(V, F)
    vs.copy_(x)
    vd.copy_(x)
    assert vs.data_ptr() % 4 != 0 or dt == F32
    assert vs.data_ptr() % 16 != 0 and vd.data_ptr() % 16 != 0 and vy.data_ptr() % 16 != 0
    keep_s, keep_d = bs.clone(), bd.clone()
    agg.run_v2(vs, vd, a, vy, heads=H)
    assert torch.equal(vy, y_shared)
    assert torch.equal(bs, keep_s) and torch.equal(bd, keep_d)
    assert (by[:1] == 7.0).all() and (by[1 + n:] == 7.0).all()
    # the flat function is the same call
    y_flat = full((V, F), dt)
    gnc.gatv2_run(agg, x, x, a, y_flat, heads=H)
    assert torch.equal(y_flat, y_shared)


# ------------------------------------------------------------------------------------------ 7. HIP graph
@pytest.mark.parametrize("H,D", [(1, 128), (8, 16), (2, 301)])
def test_graph_capture_and_replay(H, D):
    ptr, idx = GRAPHS["powerlaw"]()
    V, F = len(ptr) - 1, H * D
    xb, _, _ = bf16_pair((V, F), 51)
    a = dev(att_vec(H, D, 52))
    agg = gnc.Aggregator_GAT(dev(ptr), dev(idx), F, F)
    for ydt in (F32, B16):
        y = full((V, F), ydt)
        agg.run_v2(xb, xb, a, y, heads=H)       # warm call: the list of long rows, the scratch
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):               # (captures on a side stream: the call may neither allocate nor synchronise)
            agg.run_v2(xb, xb, a, y, heads=H)
        for seed in (53, 54):
            a.copy_(dev(att_vec(H, D, seed)))
            y.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            eager = full((V, F), ydt)
            agg.run_v2(xb, xb, a, eager, heads=H)
            assert torch.equal(y, eager) and torch.isfinite(y.float()).all()


# ------------------------------------------------------------------------------------------ 8. refusals of the C-ABI
def test_cabi_refusals_leave_y_alone():
    ptr, idx = GRAPHS["uniform"]()
    V, F = len(ptr) - 1, 16
    dptr, didx = dev(ptr), dev(idx)
    gat = gnc.Aggregator_GAT(dptr, didx, F, F)
    gcn = gnc.Aggregator_GCN(dptr, didx, None, F, F)
    big = gnc.Aggregator_GAT.GATV2_MAX_FEAT + 8
    x, a, y = torch.zeros((V, big), device=DEV), torch.zeros(big, device=DEV), full((V, big))
    L = gnc.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def refused(text, h=None, xs=x, xd=x, xt=0, av=a, yv=y, yt=0, feat=F, heads=2, slope=0.2):
        rc = L.gnnagg_gatv2_run(gat._h if h is None else h, None if xs is None else p(xs), None if xd is None else p(xd), xt,
                                None if av is None else p(av), None if yv is None else p(yv), yt, feat, heads, ctypes.c_float(slope))
        err = L.gnnagg_last_error()
        assert rc == _lib.ERR_ARG and b"gnnagg_gatv2_run" in err and text in err, err
    refused(b"not a GAT aggregator", h=gcn._h)
    refused(b"d_xs", xs=None)
    refused(b"d_xd", xd=None)
    refused(b"d_a", av=None)
    refused(b"d_y", yv=None)
    refused(b"x_dtype 7", xt=7)
    refused(b"y_dtype -1", yt=-1)
    refused(b"feat = 0", feat=0)
    refused(b"feat = -4", feat=-4)
    refused(b"heads = 0", heads=0)
    refused(b"heads = 3", heads=3)
    refused(b"slope", slope=-0.1)
    refused(b"slope", slope=1.5)
    refused(b"slope", slope=float("nan"))
    refused(("limit of %d" % gnc.Aggregator_GAT.GATV2_MAX_FEAT).encode(), feat=big, heads=1)
    torch.cuda.synchronize()
    assert (y == 7.0).all()
    # the limit itself runs
    F = gnc.Aggregator_GAT.GATV2_MAX_FEAT
    _, x32, x_np = bf16_pair((V, F), 61, 0.5)
    an = att_vec(1, F, 62) * 0.2
    ok = full((V, F))
    gat.run_v2(x32, x32, dev(an), ok, heads=1)
    ref, Lc, S = gatv2_ref(ptr, idx, x_np, x_np, an, 1, block_edges=judge_block(F))
    ratio = worst_ratio(ok.cpu().numpy(), ref, gatv2_bound(Lc, S, 1))
    print("F = %d: worst ratio %.4f" % (F, ratio))
    assert ratio <= 1.0
    with pytest.raises(gnc.GnnAggError, match="limit of"):
        gat.run_v2(x, x, a, y, heads=1)
