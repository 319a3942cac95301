"""GPU: the 3-layer forward of examples/forward_3layer.py with model "our_Transformer" (a layer: qkv = dense(feat, [Wq | Wk | Wv]), then
Aggregator_GAT.run_dot on the three column views of qkv), fp32 and bf16, one head and eight.  Every layer's attention output is judged from
its traced inputs with the float64 judge and the bound of tests/test_gpu_dot_attn.py; a bf16 output must be one rounding of the fp32-y run
on the same traced inputs, which is what is judged.  A forward replayed from a HIP graph gives the bits of the eager one."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from test_dot_attn_host import dot_attn_bound, dot_attn_ref
from test_gatv2_host import worst_ratio

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import forward_3layer as f3  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
V = 2000


def graph():
    return gnc.graph.powerlaw_csr(V, 30000, seed=123)


def model(dtype, heads):
    ptr_t, idx_t = graph()
    return f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN, dtype=dtype, heads=heads, transformer=True), ptr_t.numpy(), idx_t.numpy()


@pytest.mark.parametrize("heads", [1, 8])
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_transformer_forward_layer_by_layer(dtype, heads):
    m, ptr, idx = model(dtype, heads)
    m.trace = []
    y = m.forward("our_Transformer")
    assert len(m.trace) == 3 and y.shape == (V, 32) and y.dtype == dtype and bool(torch.isfinite(y.float()).all())
    prev = m.h
    for k, t in enumerate(m.trace):
        N = f3.DIMS[k + 1]
        assert t["feat"] is prev or torch.equal(t["feat"], prev)
        assert t["w"].shape == (f3.DIMS[k], 3 * N) and t["qkv"].shape == (V, 3 * N) and t["qkv"].dtype == dtype and t["out"].dtype == dtype
        assert torch.equal(t["qkv"], gnc.matmul_NN(t["feat"], t["w"]))
        q, kk, v = t["qkv"][:, :N], t["qkv"][:, N:2 * N], t["qkv"][:, 2 * N:]
        assert not kk.is_contiguous() and kk.stride(0) == 3 * N   # the column views themselves: no copies
        out32 = torch.full((V, N), 7.0, device=DEV)
        m.at_gat.run_dot(q, kk, v, out32, heads=heads)
        if dtype == BF:
            assert torch.equal(t["out"], out32.to(BF)), "layer %d: the bf16 output is not one rounding of the fp32 result" % k
        else:
            assert torch.equal(t["out"], out32)
        x = t["qkv"].float().cpu().numpy()
        ref, L, S = dot_attn_ref(ptr, idx, x[:, :N], x[:, N:2 * N], x[:, 2 * N:], heads, np.float32(1.0 / math.sqrt(N // heads)))
        ratio = worst_ratio(out32.cpu().numpy(), ref, dot_attn_bound(L, S, heads))
        print("layer %d (%s, %d heads): worst |y - ref| / bound = %.4f" % (k, dtype, heads, ratio))
        assert bool(torch.isfinite(out32).all()) and ratio <= 1.0, "layer %d: worst ratio %.3g" % (k, ratio)
        prev = t["out"]
    assert torch.equal(y, m.trace[-1]["out"])


@pytest.mark.parametrize("dtype,heads", [(torch.float32, 1), (BF, 8)])
def test_a_forward_replayed_from_a_hip_graph_gives_the_eager_bits(dtype, heads):
    """what --hip-graph does: one warm forward, then a captured one"""
    m, _, _ = model(dtype, heads)
    eager = m.forward("our_Transformer").clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        result = m.forward("our_Transformer")
    result.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(result, eager) and bool(torch.isfinite(result.float()).all())
    m.h.mul_(0.5)                  # new features: the replay follows them
    g.replay()
    torch.cuda.synchronize()
    replayed = result.clone()
    assert not torch.equal(replayed, eager)
    assert torch.equal(m.forward("our_Transformer"), replayed)


def test_the_other_models_keep_their_seeded_values():
    """the packed weights are drawn behind every tensor the other models seed"""
    ptr_t, idx_t = graph()
    a = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN)
    b = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), 32, 1, False, dense=gnc.matmul_NN, transformer=True)
    assert torch.equal(a.h, b.h) and not hasattr(a, "w_qkv")
    for k in range(3):
        assert torch.equal(a.weights[k], b.weights[k]) and torch.equal(a.weights_lr[k], b.weights_lr[k])
