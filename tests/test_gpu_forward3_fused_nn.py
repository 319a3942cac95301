"""GPU: the 3-layer GCN forward of examples/forward_3layer.py with fused_nn = True -- layers 0 and 1 aggregate, apply the ReLU and multiply by
the NEXT layer's weights in one call (gnnagg_gcn_run_with_nn_typed).  fp32: bit-equal, stage by stage, to the fused_relu forward with separate
dense launches (the fp32 epilogue is the library GEMM's ascending-k chain).  bf16: every stage against its own contract -- out_k the typed
aggregation + ReLU of feat2_k, feat2_{k+1} within 1e-5 . sum|y w| of the float64 product of the stored out_k and W_{k+1} and one rounding of
the fp32-transformed call."""
import os
import sys

import pytest
import torch

import gnn_computing_amd as gnc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import forward_3layer as f3  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NG = 32
KEYS = {"feat", "w", "feat2", "out"}


def model(dtype, fused_nn):
    ptr_t, idx_t = gnc.graph.powerlaw_csr(2000, 30000, seed=123)
    m = f3.Model(ptr_t.to(DEV), idx_t.to(DEV), NG, 1, True, dense=gnc.matmul_NN, dtype=dtype, fused_nn=fused_nn)
    m.trace = []
    return m


def test_gcn_forward_fp32_equals_the_unfused_forward_bit_for_bit():
    a, b = model(torch.float32, False), model(torch.float32, True)
    ya, yb = a.forward("our_GCN").clone(), b.forward("our_GCN")
    assert len(a.trace) == 3 and len(b.trace) == 3 and yb.shape == (2000, 32) and bool(torch.isfinite(yb).all())
    assert torch.equal(ya, yb)
    for k, (ta, tb) in enumerate(zip(a.trace, b.trace)):
        assert set(tb) == KEYS and set(ta) == KEYS
        for key in ("feat", "w", "feat2", "out"):
            assert torch.equal(ta[key], tb[key]), "layer %d %s" % (k, key)
    assert b.at.last_nn_path() == 1   # layer 1's call (64 -> 32) was the last: its product ran as the aggregation kernel's epilogue


def test_gcn_forward_bf16_stage_by_stage():
    m = model(BF, True)
    y = m.forward("our_GCN")
    assert len(m.trace) == 3 and y.shape == (2000, 32) and y.dtype == BF and bool(torch.isfinite(y).all())
    prev = m.h
    for k, t in enumerate(m.trace):
        assert set(t) == KEYS and all(t[key].dtype == BF for key in KEYS)
        assert t["feat"] is prev or torch.equal(t["feat"], prev)
        if k == 0:   # as today: one rounding of the fp32-out call, which is within the bound of float64
            c32 = gnc.matmul_NN(t["feat"], t["w"], out_dtype=torch.float32)
            assert torch.equal(t["feat2"], c32.to(BF))
            prod, c = t["feat"].double() @ t["w"].double(), c32
            bound = 1e-5 * (t["feat"].double().abs() @ t["w"].double().abs()) + 1e-30
        else:        # contract 3 against the stored out_{k-1} and W_k; bf16: one rounding of the fp32-transformed call on the same inputs
            src = m.trace[k - 1]
            y2 = torch.full(src["out"].shape, float("nan"), device=DEV, dtype=BF)
            c = torch.full(t["feat2"].shape, float("nan"), device=DEV)
            m.at.run_with_nn_typed(src["feat2"], y2, t["w"], c, scheduled=1, relu=True)
            assert torch.equal(y2, src["out"])
            assert torch.equal(t["feat2"], c.to(BF)), "layer %d: feat2 is not one rounding of the fp32 product" % k
            prod = src["out"].double() @ t["w"].double()
            bound = 1e-5 * (src["out"].double().abs() @ t["w"].double().abs()) + 1e-30
        err = (c.double() - prod).abs()
        print("layer %d dense: worst err / bound %.3g" % (k, float((err / bound).max().item())))
        assert bool((err <= bound).all().item()), "layer %d dense" % k
        out = torch.full(t["out"].shape, float("nan"), device=DEV, dtype=BF)
        gnc.gcn_run(m.at, t["feat2"], out, 128, 1, relu=True)
        assert torch.equal(t["out"], out), "gcn layer %d aggregation + relu" % k
        prev = t["out"]
    assert torch.equal(y, m.trace[-1]["out"])


def test_the_gat_model_ignores_fused_nn():
    a, b = model(torch.float32, False), model(torch.float32, True)
    assert torch.equal(a.forward("our_GAT"), b.forward("our_GAT"))
    assert all("att" in t for t in b.trace)
