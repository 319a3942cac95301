"""GPU: the 3-layer forward of examples/forward_3layer.py with model "our_GATv2" (a layer: feat2 = dense(feat, W), then Aggregator_GAT.run_v2 on
feat2 for both sides), fp32 and bf16, one head and eight.  Every layer's output is judged from its traced inputs with the float64 judge and the
bound of tests/test_gpu_gatv2.py; a bf16 output must be one rounding of the fp32-y run on the same traced inputs, which is what is judged."""
import os
import sys

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from test_gatv2_host import gatv2_bound, gatv2_ref, worst_ratio

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import forward_3layer as f3  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
V = 2000


def graph():
    return gnc.graph.powerlaw_csr(V, 30000, seed=123)


@pytest.mark.parametrize("heads", [1, 8])
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_gatv2_forward_layer_by_layer(dtype, heads):
    ptr_t, idx_t = graph()
    ptr, idx = ptr_t.numpy(), idx_t.numpy()
    m = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN, dtype=dtype, heads=heads, gatv2=True)
    m.trace = []
    y = m.forward("our_GATv2")
    assert len(m.trace) == 3 and y.shape == (V, 32) and y.dtype == dtype and bool(torch.isfinite(y.float()).all())
    prev = m.h
    for k, t in enumerate(m.trace):
        N = f3.DIMS[k + 1]
        assert t["feat"] is prev or torch.equal(t["feat"], prev)
        assert t["feat2"].dtype == dtype and t["out"].dtype == dtype and t["a"].dtype == torch.float32 and t["a"].shape == (heads, N // heads)
        assert torch.equal(t["feat2"], gnc.matmul_NN(t["feat"], t["w"]))
        out32 = torch.full((V, N), 7.0, device=DEV)
        m.at_gat.run_v2(t["feat2"], t["feat2"], t["a"], out32, heads=heads)
        if dtype == BF:
            assert torch.equal(t["out"], out32.to(BF)), "layer %d: the bf16 output is not one rounding of the fp32 result" % k
        else:
            assert torch.equal(t["out"], out32)
        x = t["feat2"].float().cpu().numpy()
        ref, L, S = gatv2_ref(ptr, idx, x, x, t["a"].cpu().numpy(), heads)
        ratio = worst_ratio(out32.cpu().numpy(), ref, gatv2_bound(L, S, heads))
        print("layer %d (%s, %d heads): worst |y - ref| / bound = %.4f" % (k, dtype, heads, ratio))
        assert bool(torch.isfinite(out32).all()) and ratio <= 1.0, "layer %d: worst ratio %.3g" % (k, ratio)
        prev = t["out"]
    assert torch.equal(y, m.trace[-1]["out"])


def test_the_other_models_keep_their_seeded_values():
    """a_k is drawn behind every tensor the other models seed"""
    ptr_t, idx_t = graph()
    a = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN)
    b = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN, gatv2=True)
    assert torch.equal(a.h, b.h) and not hasattr(a, "a_v2")
    for k in range(3):
        assert torch.equal(a.weights[k], b.weights[k]) and torch.equal(a.weights_lr[k], b.weights_lr[k])
