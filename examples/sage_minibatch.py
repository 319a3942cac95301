#!/usr/bin/env python3
"""Mini-batch GraphSAGE forward (2 layers, mean aggregation) over sampled blocks: sample on the device (gnc.NeighborSampler), gather the
input rows, and per layer h_dst' = relu(h_dst . W_self + mean_{kept neighbours}(h_src) . W_neigh) with the library's aggregation and GEMM.

    python examples/sage_minibatch.py [--dataset arxiv] [--batch 1024] [--fanouts 15,10] [--batches 20] [--weighted] [--block-run]

--weighted draws the neighbours in proportion to a per-edge weight (NeighborSampler(prob=); a third of the edges have weight 0 and are never
drawn) and aggregates the weighted sum with the kept edges' own weights, full_val[blk.eid].

Prints one JSON line with the per-stage times (medians over the batches, microseconds, each stage closed by a device synchronisation).  A
block is a new graph, so every batch creates its aggregators: the "aggregate" stage holds handle creation, plan and run.

--block-run aggregates every block with one launch instead (Block.aggregate): no handle, no plan, and no gather stage -- the input layer
reads x in place through blocks[0].src_nodes and returns x_dst beside the aggregate; --weighted then passes the full per-edge values and
lets the call read them through blk.eid (val_full=True).  The JSON line gains "block_run": true and its "gather_us" is 0."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gnn_computing_amd as gnc  # noqa: E402

DIMS = [128, 128, 64]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="arxiv")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fanouts", default="15,10", help="input layer first")
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weighted", action="store_true", help="sample by a per-edge weight and aggregate with it")
    ap.add_argument("--block-run", action="store_true", help="aggregate each block with one Block.aggregate call: no handle, no gather")
    args = ap.parse_args()
    fanouts = tuple(int(f) for f in args.fanouts.split(","))
    assert len(fanouts) == 2, "this example has two layers"
    dev = torch.device("cuda", 0)
    ptrs, idxs = gnc.graph.dataset(args.dataset, device=dev)
    num_v = ptrs.numel() - 1
    gen = torch.Generator().manual_seed(123)
    x = torch.randn(num_v, DIMS[0], generator=gen).to(dev)
    w_self = [(torch.randn(DIMS[k], DIMS[k + 1], generator=gen) / DIMS[k] ** 0.5).to(dev) for k in range(2)]
    w_neigh = [(torch.randn(DIMS[k], DIMS[k + 1], generator=gen) / DIMS[k] ** 0.5).to(dev) for k in range(2)]
    full_val = None
    if args.weighted:
        full_val = torch.exp2(12.0 * torch.rand(idxs.numel(), generator=gen) - 6.0)
        full_val[torch.rand(idxs.numel(), generator=gen) < 1.0 / 3.0] = 0.0
        full_val = full_val.to(dev)
    sampler = gnc.NeighborSampler(ptrs, idxs, prob=full_val)
    perm = torch.randperm(num_v, generator=gen).to(torch.int32).to(dev)
    stages = {"sample": [], "gather": [], "aggregate": [], "dense": []}

    def timed(fn):
        """(result, microseconds), closed by a device synchronisation"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e6

    out = None
    for b in range(args.batches + 1):            # (batch 0 warms the allocator and the kernels up; its times are dropped)
        seeds = perm[(b * args.batch) % num_v:][:args.batch].contiguous()
        # the sample of a row depends on (seed, row) only: a new seed per batch draws a new sample
        blocks, t_sample = timed(lambda: sampler.sample_layers(seeds, fanouts, seed=args.seed + 2 * b, return_eid=args.weighted))
        reduce = "sum" if args.weighted else "mean"
        if args.block_run:
            h, t_gather = x, 0.0                      # no gather stage: layer 0 reads x in place through src_nodes
        else:
            h, t_gather = timed(lambda: x[blocks[0].src_nodes.long()])
        t_agg = t_dense = 0.0
        for k, blk in enumerate(blocks):

            def aggregate():
                y = torch.empty((blk.num_dst, h.shape[1]), device=dev)
                agg = blk.gcn(full_val[blk.eid.long()].contiguous() if args.weighted else None)
                agg.run(h, y, 512, 0, reduce=reduce)
                return y, h[:blk.num_dst], agg

            def aggregate_block_run():
                kw = {"val": full_val, "val_full": True} if args.weighted else {}
                if k == 0:                            # the aggregate and x_dst = x[src_nodes[:num_dst]] from one launch
                    return blk.aggregate(h, reduce=reduce, return_dst=True, **kw) + (None,)
                return blk.aggregate(h, reduce=reduce, gathered=True, **kw), h[:blk.num_dst], None

            (y, h_dst, agg), dt = timed(aggregate_block_run if args.block_run else aggregate)
            t_agg += dt
            h, dt = timed(lambda: F.relu(gnc.matmul_NN(h_dst.contiguous(), w_self[k]) + gnc.matmul_NN(y, w_neigh[k])))
            t_dense += dt
            if agg is not None:
                agg.close()
        if b > 0:
            for stage, dt in (("sample", t_sample), ("gather", t_gather), ("aggregate", t_agg), ("dense", t_dense)):
                stages[stage].append(dt)
        out = h
    rec = {"model": "sage_minibatch", "dataset": args.dataset, "num_v": num_v, "num_e": idxs.numel(), "batch": args.batch, "fanouts": list(fanouts), "weighted": args.weighted,
           "batches": args.batches, "last_blocks": [[blk.num_dst, blk.num_src, blk.num_edges] for blk in blocks],
           "finite": bool(torch.isfinite(out).all().item())}
    if args.block_run:
        rec["block_run"] = True
    rec.update({k + "_us": statistics.median(v) for k, v in stages.items()})
    rec["total_us"] = sum(rec[k + "_us"] for k in stages)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
