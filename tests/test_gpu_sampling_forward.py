"""GPU: sampled blocks through the aggregators.  With every edge kept, two hops over the blocks are the seed rows of two hops over the full
graph bit for bit (a sampled row keeps CSR order and `scheduled = 0` runs the canonical chain); with fanout 5 each block's mean is the
float64 mean over the restatement's kept edges inside the project's 1e-5 bound; blk.eid gathers the per-edge values of a weighted run."""
import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc

import sampling_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PTR, IDX = sr.fixture_graph()
V, E = len(PTR) - 1, len(IDX)
F = 32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def seeds_of_the_test():
    rng = np.random.default_rng(4)
    return np.concatenate([sr.crafted_rows(), rng.choice(V, 200, replace=False)]).astype(np.int32)


def features():
    return np.random.default_rng(5).standard_normal((V, F)).astype(np.float32)


def run(agg, x, rows, reduce):
    y = torch.full((rows, x.shape[1]), 7.0, device=DEV)
    agg.run(x, y, 512, 0, reduce=reduce)
    return y


def run_block(blk, x, reduce, val=None):
    agg = blk.gcn(val)
    y = run(agg, x, blk.num_dst, reduce)
    torch.cuda.synchronize()
    agg.close()
    return y


def test_two_hops_with_every_edge_kept_are_the_full_graph_bit_for_bit():
    ptr, idx, x = dev(PTR), dev(IDX), dev(features())
    full = gnc.Aggregator_GCN(ptr, idx, None)
    h2 = run(full, run(full, x, V, "mean"), V, "mean")
    torch.cuda.synchronize()
    full.close()
    seeds = dev(seeds_of_the_test())
    sampler = gnc.NeighborSampler(ptr, idx)
    blocks = sampler.sample_layers(seeds, fanouts=(-1, -1), seed=0)
    sampler.close()
    assert blocks[0].num_dst == blocks[1].num_src and blocks[1].num_dst == len(seeds)
    h = x[blocks[0].src_nodes.long()]
    for blk in blocks:
        h = run_block(blk, h.contiguous(), "mean")
    assert torch.equal(h.view(torch.int32), h2[seeds.long()].view(torch.int32))


def mean64(blk_ptr, blk_idx, x_src):
    """(float64 mean over the block's edges, mean of |x| over them) per row"""
    n = len(blk_ptr) - 1
    out, scale = np.zeros((n, x_src.shape[1])), np.zeros((n, x_src.shape[1]))
    x64 = x_src.astype(np.float64)
    for i in range(n):
        nb = blk_idx[blk_ptr[i]:blk_ptr[i + 1]]
        if len(nb):
            out[i], scale[i] = x64[nb].mean(0), np.abs(x64[nb]).mean(0)
    return out, scale


def test_fanout_5_blocks_are_the_mean_over_the_kept_edges():
    ptr, idx, x = dev(PTR), dev(IDX), features()
    seeds = seeds_of_the_test()
    sampler = gnc.NeighborSampler(ptr, idx)
    blocks = sampler.sample_layers(dev(seeds), fanouts=(5, 5), seed=20)
    sampler.close()
    # the restatement's blocks: the output layer from the seeds with seed + 1, the input layer from its source rows with seed + 0
    top = sr.sample_block(PTR, IDX, seeds, 5, 21, True)
    low = sr.sample_block(PTR, IDX, top[3], 5, 20, True)
    h = x[low[3]]
    assert np.array_equal(blocks[0].src_nodes.cpu().numpy(), low[3])
    for blk, r in zip(blocks, (low, top)):
        assert np.array_equal(blk.ptr.cpu().numpy(), r[0]) and np.array_equal(blk.idx.cpu().numpy(), r[1])
        y = run_block(blk, dev(h), "mean").cpu().numpy()
        want, scale = mean64(r[0], r[1], h)      # of the fp32 rows this block was given
        err = np.abs(y - want)
        print("worst |y - mean64| / (1e-5 * mean |x|) = %.4f" % float((err / np.maximum(1e-5 * scale, 1e-300)).max()))
        assert (err <= 1e-5 * scale).all()
        h = y


def test_eid_gathers_the_values_of_a_weighted_full_graph_run():
    ptr, idx, x = dev(PTR), dev(IDX), dev(features())
    val = dev(np.random.default_rng(6).standard_normal(E).astype(np.float32))
    full = gnc.Aggregator_GCN(ptr, idx, val)
    y_full = run(full, x, V, "sum")
    seeds = dev(seeds_of_the_test())
    sampler = gnc.NeighborSampler(ptr, idx)
    blk = sampler.sample(seeds, -1, seed=3, relabel=True, return_eid=True)
    sampler.close()
    assert torch.equal(idx[blk.eid.long()], blk.src_nodes[blk.idx.long()])
    y = run_block(blk, x[blk.src_nodes.long()].contiguous(), "sum", val[blk.eid.long()].contiguous())
    assert torch.equal(y.view(torch.int32), y_full[seeds.long()].view(torch.int32))
    full.close()


def test_a_block_without_edges_aggregates_to_zero():
    """seeds that are rows without edges: idx is a zero-length slice, the aggregators take it"""
    ptr, idx, x = dev(PTR), dev(IDX), dev(features())
    rows = np.flatnonzero(np.diff(PTR) == 0)[:3].astype(np.int32)
    assert len(rows) == 3
    sampler = gnc.NeighborSampler(ptr, idx)
    blk = sampler.sample(dev(rows), 5, seed=1, return_eid=True)
    sampler.close()
    assert (blk.num_dst, blk.num_src, blk.num_edges) == (3, 3, 0) and blk.idx.numel() == 0 and blk.eid.numel() == 0
    for reduce in ("sum", "mean"):
        y = run_block(blk, x[blk.src_nodes.long()].contiguous(), reduce)
        assert (y == 0).all().item()
    gat = blk.gat()
    gat.close()
