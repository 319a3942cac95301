"""Host: the float64 references of tests/test_gpu_large.py (plain gather-and-reduce in row blocks, the GAT bound, the compacted problem)
against the CPU oracle on a small graph, so that the checker of the large-size tests is itself checked without a GPU."""
import numpy as np
import pytest
import torch

import test_gpu_large as big
from oracle import oracle as orc


@pytest.fixture()
def small(monkeypatch):
    monkeypatch.setattr(big, "DEV", "cpu")
    G = big.rect_graph(300, 6000, 5000, seed=3, hub_deg=20000)   # the last row (and two more) above the block size and the heavy-row cut
    blocks = G.blocks
    G.blocks = lambda max_edges=5000, heavy=1 << 14: blocks(max_edges, heavy)
    x = big.ints((G.cols, 8), big.gen(1))
    return G, x


def test_row_blocks_cover_every_row_once(small):
    G, _ = small
    seen = np.zeros(G.V, int)
    for r0, r1 in G.blocks():
        seen[r0:r1] += 1
    assert (seen == 1).all() and len(list(G.blocks())) > 4


@pytest.mark.parametrize("reduce", ["sum", "max", "mean"])
def test_gcn_reference_is_the_oracle_on_integers(small, reduce):
    G, x = small
    fn = {"sum": orc.gcn_seq, "max": orc.gcn_max, "mean": orc.gcn_mean}[reduce]
    y = torch.from_numpy(fn(G.ptr_h.astype(np.int32), G.idx.numpy(), G.val.numpy(), x.numpy()))
    big.check_gcn(y, G, x, G.val, reduce, reduce=reduce)
    for r, c in ((G.V - 1, 3), (0, 0), (150, 7)):       # a wrong integer or a NaN anywhere fails
        for bad in (y[r, c] + 1, float("nan")):
            y2 = y.clone()
            y2[r, c] = bad
            with pytest.raises(AssertionError):
                big.check_gcn(y2, G, x, G.val, reduce, reduce=reduce)


@pytest.mark.parametrize("H", [1, 4])
def test_gat_reference_and_compaction_agree_with_the_oracle(small, H):
    G, x = small
    att = torch.randn((G.cols, H, 2), generator=big.gen(2)) * 0.5
    ptr, idx = G.ptr_h.astype(np.int32), G.idx.numpy()
    y = torch.from_numpy(orc.gat_fused(ptr, idx, att.numpy(), x.numpy(), H))
    big.check_gat(y, G, x, att, H, "gat")
    C, xc, att_c = big.compacted(G, x, att, H)
    assert C.cols < G.cols
    big.check_gat(y, C, xc, att_c, H, "gat on the compacted problem")
    for bad in (y[5, 2] + 0.01, float("nan")):
        y2 = y.clone()
        y2[5, 2] = bad
        with pytest.raises(AssertionError):
            big.check_gat(y2, G, x, att, H, "gat")
