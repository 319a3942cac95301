"""GPU: the 3-layer GAT forward of examples/forward_3layer.py with fused_project=True (gnc.gat_project in front of every aggregation), checked
layer by layer on the traced tensors: feat2 bit-equal to matmul_NN on the layer's input, the attention terms within 1e-5 . sum|feat2 . a| of
float64 on the stored feat2, and the layer's output bit-equal to a separate aggregation of the traced (feat2, att).  fp32 and bf16, one
head and eight (head widths 16, 8 and 4: the last one is outside what the GEMM kernel's epilogue reduces and takes the row-dot kernel)."""
import os
import sys

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import forward_3layer as f3  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
RTOL = 1e-5
NG = 32
V = 2000


def model(dtype, heads, fused_project=True):
    ptr_t, idx_t = gnc.graph.powerlaw_csr(V, 30000, seed=123)
    m = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), NG, 1, False, dense=gnc.matmul_NN, dtype=dtype, fused_project=fused_project, heads=heads)
    m.trace = []
    return m


@pytest.mark.parametrize("heads", [1, 8])
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_gat_forward_with_fused_project_layer_by_layer(dtype, heads):
    m = model(dtype, heads)
    y = m.forward("our_GAT")
    assert len(m.trace) == 3 and y.shape == (V, 32) and y.dtype == dtype and bool(torch.isfinite(y).all())
    prev = m.h
    for k, t in enumerate(m.trace):
        N = f3.DIMS[k + 1]
        D = N // heads
        assert t["feat"] is prev or torch.equal(t["feat"], prev)
        assert t["feat2"].dtype == dtype and t["att"].dtype == torch.float32 and t["att"].shape == (V, heads, 2) and t["out"].dtype == dtype
        assert torch.equal(t["feat2"], gnc.matmul_NN(t["feat"], t["w"])), "layer %d: feat2 is not what matmul_NN writes" % k
        assert t["path"] == (1 if dtype == BF and (heads == 1 or D in (8, 16, 32, 64)) else 2), "layer %d" % k
        f = t["feat2"].double().cpu().numpy().reshape(V, heads, D)
        a = np.stack([t["a_dst"].double().cpu().numpy().reshape(heads, D), t["a_src"].double().cpu().numpy().reshape(heads, D)], axis=-1)
        ref, scale = np.einsum("mhd,hdt->mht", f, a), np.einsum("mhd,hdt->mht", np.abs(f), np.abs(a))
        err = np.abs(t["att"].double().cpu().numpy() - ref)
        assert (err <= RTOL * scale + 1e-30).all(), "layer %d: att outside 1e-5 * sum|feat2 a| (worst ratio %.3g)" % (k, float((err / (scale + 1e-300)).max()))
        out = torch.full_like(t["out"], float("nan"))
        m.at_gat.run(t["feat2"], t["att"], out, 128, 1, heads=heads)
        assert torch.equal(t["out"], out), "layer %d: the aggregation of the traced (feat2, att)" % k
        prev = t["out"]
    assert torch.equal(y, m.trace[-1]["out"])


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_one_head_uses_the_columns_of_w_lr_and_the_default_model_is_unchanged(dtype):
    """a_dst = w_lr[:, 0], a_src = w_lr[:, 1]; without the keyword the model has the weights, the input and the layers it had"""
    a, b = model(dtype, 1, fused_project=False), model(dtype, 1)
    assert not a.fused_project and torch.equal(a.h, b.h)
    for k in range(3):
        assert torch.equal(a.weights[k], b.weights[k]) and torch.equal(a.weights_lr[k], b.weights_lr[k])
        assert torch.equal(b.a_dst[k], b.weights_lr[k][:, 0]) and torch.equal(b.a_src[k], b.weights_lr[k][:, 1])
    a.forward("our_GAT")
    b.forward("our_GAT")
    for ta, tb in zip(a.trace, b.trace):
        if ta is a.trace[0]:
            assert torch.equal(ta["feat2"], tb["feat2"])   # the same first projection; later layers see att in another summation order
        assert "w_lr" in ta and "a_dst" in tb


def test_more_than_one_head_needs_gat_project():
    ptr_t, idx_t = gnc.graph.powerlaw_csr(V, 30000, seed=123)
    with pytest.raises(ValueError, match="fused_project"):
        f3.Model(ptr_t.to(DEV), idx_t.to(DEV), NG, 1, False, dense=gnc.matmul_NN, heads=8)
