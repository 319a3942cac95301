"""GPU: the 3-layer forward of examples/forward_3layer.py with model "our_PNA" (a layer: relu(dense(cat[x, multi(x)], W)) with multi =
Aggregator_GCN.run_multi -- mean, min, max and std of the neighbourhood, identity scaler), fp32 and bf16.  Every layer's aggregation is
judged from its traced input with the float64 reference and the bounds of tests/test_gpu_multi_aggr.py; a bf16 block must be one rounding
of the fp32-y run on the same traced input, which is what is judged; the dense part must be the library's own product of the traced
concatenation.  A forward replayed from a HIP graph gives the bits of the eager one."""
import os
import sys

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from test_multi_aggr_host import BOUNDS, multi_layout, multi_ref, worst_ratio

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import forward_3layer as f3  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
V = 2000
PNA_AGGRS = ("mean", "min", "max", "std")


def graph():
    return gnc.graph.powerlaw_csr(V, 30000, seed=123)


def model(dtype):
    ptr_t, idx_t = graph()
    return f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN, dtype=dtype), ptr_t.numpy(), idx_t.numpy()


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_pna_forward_layer_by_layer(dtype):
    m, ptr, idx = model(dtype)
    m.trace = []
    y = m.forward("our_PNA")
    assert len(m.trace) == 3 and y.shape == (V, 32) and y.dtype == dtype and bool(torch.isfinite(y.float()).all())
    prev = m.h
    for k, t in enumerate(m.trace):
        N = f3.DIMS[k]
        assert t["feat"] is prev or torch.equal(t["feat"], prev)
        assert t["w"].shape == (5 * N, f3.DIMS[k + 1]) and t["multi"].shape == (V, 4 * N) and t["multi"].dtype == dtype
        out32 = torch.full((V, 4 * N), 7.0, device=DEV)
        m.at.run_multi(t["feat"], out32, aggrs=PNA_AGGRS)
        if dtype == BF:
            assert torch.equal(t["multi"], out32.to(BF)), "layer %d: the bf16 blocks are not one rounding of the fp32 result" % k
        else:
            assert torch.equal(t["multi"], out32)
        ref = multi_ref(ptr, idx, np.ones(len(idx), np.float32), t["feat"].float().cpu().numpy())
        got = out32.cpu().numpy()
        for (_, a), cols in multi_layout(PNA_AGGRS, ("identity",), N).items():
            if a in ("min", "max"):
                assert np.array_equal(got[:, cols], ref[a]), "layer %d: %s is not exact" % (k, a)
            else:
                ratio = worst_ratio(got[:, cols], ref[a], BOUNDS[a](ref))
                print("layer %d (%s): %s worst |y - ref| / bound = %.4f" % (k, dtype, a, ratio))
                assert ratio <= 1.0, "layer %d: %s worst ratio %.3g" % (k, a, ratio)
        assert torch.equal(t["cat"], torch.cat([t["feat"], t["multi"]], 1))
        assert torch.equal(t["out"], torch.relu(gnc.matmul_NN(t["cat"], t["w"]))) and t["out"].dtype == dtype
        prev = t["out"]
    assert torch.equal(y, m.trace[-1]["out"])


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_a_forward_replayed_from_a_hip_graph_gives_the_eager_bits(dtype):
    """what --hip-graph does: one warm forward, then a captured one"""
    m, _, _ = model(dtype)
    eager = m.forward("our_PNA").clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        result = m.forward("our_PNA")
    result.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(result, eager) and bool(torch.isfinite(result.float()).all())
    m.h.mul_(0.5)                  # new features: the replay follows them
    g.replay()
    torch.cuda.synchronize()
    replayed = result.clone()
    assert not torch.equal(replayed, eager)
    assert torch.equal(m.forward("our_PNA"), replayed)


def test_the_other_models_keep_their_seeded_values():
    """the PNA weights come from a generator of their own, on the first PNA forward"""
    ptr_t, idx_t = graph()
    a = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN)
    b = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN)
    assert a.w_pna is None and b.w_pna is None
    b.forward("our_PNA")
    assert len(b.w_pna) == 3 and a.w_pna is None and torch.equal(a.h, b.h)
    for k in range(3):
        assert torch.equal(a.weights[k], b.weights[k]) and torch.equal(a.weights_lr[k], b.weights_lr[k])
