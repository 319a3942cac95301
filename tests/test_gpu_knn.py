"""GPU: knn_graph / gnnagg_knn_run (include/gnnagg.h section I, "kNN graph") against float64 numpy: distances by the same formula, then
np.lexsort((j, d)) (test_knn_host.knn_ref).
Exact cases: integer points in [-4, 4] are exact in bf16 and in every fp32 product and sum up to F = 256, so idx, ptr and dist must EQUAL
the reference, ties included.  Random floats: near-ties may legitimately reorder, so a row is judged by distance.  With S_ij = |x_i|^2 +
|y_j|^2 + 2 sum_c |x_ic y_jc| every fp32 sum of the expansion, in any order, lies within B_ij = (F + 4) 2^-24 S_ij of d_ij (gamma_n with
n = F + 4 >= the F products and additions of a term and the three of the expansion).  Measured on one MI355X (profiles/knn/gpu_tests_output.txt): the worst |dist - d64| / B of this file is 0.215 (fp32, F = 3), 0.144 (bf16, F = 3)
and at most 0.035 for F = 64 and 200."""
import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc

from test_knn_host import knn_ref, layout_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32, B16 = torch.float32, torch.bfloat16
PAD, CANARY = 64, -7
dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)

# (layout, F, k, dtype, loop, splits): every F with both types on the straddling layout, then k, loop, splits and the layouts one at a time
EXACT = [("straddle", F, 20, dt, False, 0) for F in (1, 3, 4, 5, 64, 67, 256) for dt in (F32, B16)] + [
    ("cloud", 64, 1, F32, False, 0), ("cloud", 64, 64, B16, False, 3), ("cloud", 67, 64, F32, True, 3), ("cloud", 256, 20, F32, False, 3),
    ("straddle", 64, 20, F32, True, 3), ("straddle", 5, 64, B16, True, 0), ("one", 3, 1, F32, False, 0), ("one", 3, 20, F32, True, 3),
    ("short", 4, 20, B16, False, 0), ("short", 64, 20, F32, True, 3), ("bipartite", 67, 20, F32, False, 0), ("bipartite", 64, 20, B16, False, 3),
]


def run_with_canaries(x, k, xp, y=None, yp=None, loop=False, splits=0):
    """gnnagg_knn_run into buffers with margins of PAD canaries on both sides: (ptr, idx, dist) as numpy, the margins checked"""
    m = len(x) if y is None else len(y)
    out_ptr = gnc.knn_out_ptr(len(x), m, k, xp, yp, y is None and not loop).to(torch.int32)
    E = int(out_ptr[-1])
    ibuf = torch.full((E + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)
    dbuf = torch.full((E + 2 * PAD,), float(CANARY), dtype=torch.float32, device=DEV)
    gnc.knn_run(x, k, out_ptr, ibuf[PAD:PAD + E], dbuf[PAD:PAD + E], ptr=xp, y=y, y_ptr=yp, loop=loop, splits=splits)
    for buf in (ibuf, dbuf):
        assert bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + E:] == CANARY).all()), "a margin was written"
    return out_ptr.cpu().numpy(), ibuf[PAD:PAD + E].cpu().numpy(), dbuf[PAD:PAD + E].cpu().numpy()


@pytest.mark.parametrize("name,F,k,dt,loop,splits", EXACT, ids=["%s-F%d-k%d-%s-loop%d-S%d" % (c[0], c[1], c[2], str(c[3])[6:], c[4], c[5]) for c in EXACT])
def test_integer_points_equal_the_reference(name, F, k, dt, loop, splits):
    x, y, xp, yp = layout_case(name, F)
    rp, ri, rd = knn_ref(x, x if y is None else y, k, xp, yp, y is None and not loop)
    ty = None if y is None else dev(y).to(dt)
    p, i, d = run_with_canaries(dev(x).to(dt), k, dev(xp), ty, None if y is None else dev(yp), loop, splits)
    assert np.array_equal(p, rp) and np.array_equal(i, ri) and np.array_equal(d.astype(np.float64), rd)


@pytest.mark.parametrize("dt", [F32, B16])
def test_a_row_pitched_view_through_knn_graph(dt):
    x, _, xp, yp = layout_case("straddle", 67)
    big = torch.zeros((len(x), 67 + 5), dtype=dt, device=DEV)
    big[:, 3:70] = dev(x).to(dt)
    rp, ri, rd = knn_ref(x, x, 20, xp, yp, True)
    blk, dist = gnc.knn_graph(big[:, 3:70], 20, ptr=dev(xp), return_dist=True, fused=True)
    assert (blk.num_dst, blk.num_src, blk.num_edges, blk.src_nodes, blk.eid) == (len(x), len(x), len(ri), None, None)
    assert np.array_equal(blk.ptr.cpu().numpy(), rp) and np.array_equal(blk.idx.cpu().numpy(), ri) and np.array_equal(dist.cpu().numpy(), rd)
    same = gnc.knn_graph(big[:, 3:70], 20, ptr=dev(xp), fused=False)
    assert torch.equal(same.idx, blk.idx) and torch.equal(same.ptr, blk.ptr)


@pytest.mark.parametrize("F", [3, 64, 200])
@pytest.mark.parametrize("dt", [F32, B16], ids=["float32", "bfloat16"])
def test_random_points_are_judged_by_distance(F, dt):
    k, xp = 20, np.array([0, 257, 357], np.int32)
    tx = dev(np.random.default_rng(F).standard_normal((357, F)).astype(np.float32)).to(dt)
    x = tx.float().cpu().numpy().astype(np.float64)   # the stored operands
    blk, dist = gnc.knn_graph(tx, k, ptr=dev(xp), return_dist=True, fused=True)
    idx, dist = blk.idx.cpu().numpy().reshape(357, k), dist.cpu().numpy().astype(np.float64).reshape(357, k)
    nn = (x * x).sum(1)
    worst = 0.0
    for i in range(357):
        a, b = (0, 257) if i < 257 else (257, 357)
        d64 = np.maximum(nn[i] + nn[a:b] - 2.0 * x[a:b] @ x[i], 0.0)
        bound = (F + 4) * 2.0 ** -24 * (nn[i] + nn[a:b] + 2.0 * np.abs(x[a:b]) @ np.abs(x[i]))
        j = idx[i]
        assert len(set(j)) == k and j.min() >= a and j.max() < b and i not in j
        err = np.abs(dist[i] - d64[j - a])
        worst = max(worst, float((err / bound[j - a]).max()))
        assert (err <= bound[j - a]).all() and (np.diff(dist[i]) >= 0).all()
        others = np.delete(d64, i - a)
        assert d64[j - a].max() <= np.sort(others)[k - 1] + 2.0 * np.delete(bound, i - a).max()
    print("worst err / bound, F = %d %s: %.4f" % (F, dt, worst))


def test_a_captured_call_replays_to_the_eager_bits():
    x, _, xp, _ = layout_case("cloud", 64)
    tx, tp, k, S = dev(x), dev(xp), 20, 3
    out_ptr = gnc.knn_out_ptr(300, 300, k, tp, None, True).to(torch.int32)
    work = torch.empty(gnc.knn_work_bytes(300, 300, 64, k, F32, 1, S), dtype=torch.uint8, device=DEV)
    bufs = [(torch.zeros(300 * k, dtype=torch.int32, device=DEV), torch.zeros(300 * k, dtype=torch.float32, device=DEV)) for _ in range(2)]
    gnc.knn_run(tx, k, out_ptr, *bufs[0], ptr=tp, splits=S, work=work)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        gnc.knn_run(tx, k, out_ptr, *bufs[1], ptr=tp, splits=S, work=work)
    for _ in range(3):
        bufs[1][0].zero_()
        bufs[1][1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1], bufs[1][1])
    assert np.array_equal(bufs[0][0].cpu().numpy(), knn_ref(x, x, k, xp, xp, True)[1])
