#!/usr/bin/env python3
"""Neighbour sampling (gnc.NeighborSampler; gnnagg_sampler_sample) against what a caller composed before it: two-layer mini-batches of the
arxiv- and products-shaped graphs, batches of 1 024 and 8 192 seeds and all rows, fanouts 10 and 25.  Arms:

    global      (a) the two blocks WITHOUT relabelling (global ids), over the two seed lists arm (b) samples from
    relabel     (b) sample_layers(seeds, (f, f), return_eid=True): relabelled blocks with edge positions
    torch       (c) the same two blocks composed from torch ops in this process: expand the seed rows, random keys, sort by (row, key), keep
                rank < fanout, torch.unique with inverse for the relabelling.  Its output is checked to be a VALID block (counts, every kept
                edge inside its row and kept once, ids consistent); it is sorted-id relabelling, not seeds-first, and rows are not put back
                into CSR order -- both in its favour
    host        (d) gnnagg_sample_block_host, the same two layers, on OMP_NUM_THREADS threads (16 unless the caller set it)
    handle      (e) for the input-layer block of (b): Aggregator_GCN creation + first run(mean, F = 128), and the steady run -- what a per-batch
                handle costs today (reported, not improved here)

Arms (a)-(c) alternate inside every round on a non-null stream; a round times `--calls` back-to-back calls of one arm (wall clock around a
stream synchronisation: every arm reads sizes back, so the host is part of what is measured); the figure of an arm is the median over
`--rounds` rounds, printed with the minimum and maximum of a round.  (b) is checked against the host sampler bit for bit on every shape.
One JSON line per (graph, batch, fanout); nothing is asserted about speed.

    python scripts/bench_sampling.py [--rounds 9] [--calls 20] [--datasets arxiv,products] [--batches 1024,8192,all] [--fanouts 10,25]"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--datasets", default="arxiv,products")
    ap.add_argument("--batches", default="1024,8192,all")
    ap.add_argument("--fanouts", default="10,25")
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_sampling.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()

    def torch_block(ptr, idx, seeds, fanout):
        sl = seeds.long()
        beg = ptr[sl].long()
        deg = ptr[sl + 1].long() - beg
        n = sl.numel()
        row = torch.repeat_interleave(torch.arange(n, device=dev), deg)
        start = torch.cumsum(deg, 0) - deg
        total = row.numel()
        pos = beg[row] + (torch.arange(total, device=dev) - start[row])
        o1 = torch.argsort(torch.rand(total, device=dev))
        srow, o2 = torch.sort(row[o1], stable=True)
        keep = (torch.arange(total, device=dev) - start[srow]) < fanout
        eid, krow = pos[o1[o2]][keep], srow[keep]
        blk_ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(torch.clamp(deg, max=fanout), 0)])
        src, inv = torch.unique(torch.cat([sl, idx[eid].long()]), return_inverse=True)
        return blk_ptr, inv[n:], eid, src, inv[:n], krow

    def torch_layers(ptr, idx, seeds, fanout):
        top = torch_block(ptr, idx, seeds, fanout)
        return torch_block(ptr, idx, top[3], fanout), top

    def check_torch_block(ptr_np, idx_np, seeds_np, fanout, blk):
        blk_ptr, bidx, eid, src, dst, krow = (t.cpu().numpy() for t in blk)
        deg = ptr_np[seeds_np + 1] - ptr_np[seeds_np]
        assert np.array_equal(np.diff(blk_ptr), np.minimum(deg, fanout)) and blk_ptr[-1] == len(eid)
        assert np.array_equal(krow, np.repeat(np.arange(len(seeds_np)), np.diff(blk_ptr)))
        r = seeds_np[krow]
        assert ((eid >= ptr_np[r]) & (eid < ptr_np[r + 1])).all()
        assert len(np.unique(eid)) == len(eid)      # (the seed rows are distinct, so are their edge ranges)
        assert np.array_equal(src[bidx], idx_np[eid]) and np.array_equal(src[dst], seeds_np) and len(np.unique(src)) == len(src)

    def time_round(fn, calls):
        stream.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            for _ in range(calls):
                fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls

    for name in args.datasets.split(","):
        ptrs, idxs = gnc.graph.dataset(name, device=dev)
        V, E = ptrs.numel() - 1, idxs.numel()
        ptr_np, idx_np = ptrs.cpu().numpy(), idxs.cpu().numpy()
        sampler = gnc.NeighborSampler(ptrs, idxs)
        for batch in args.batches.split(","):
            n = V if batch == "all" else min(int(batch), V)
            seeds_np = (np.arange(V) if n == V else np.random.default_rng(11).choice(V, n, replace=False)).astype(np.int32)
            seeds = torch.from_numpy(seeds_np).to(dev)
            for fanout in (int(f) for f in args.fanouts.split(",")):
                with torch.cuda.stream(stream):
                    blocks = sampler.sample_layers(seeds, (fanout, fanout), seed=1, return_eid=True)
                    seeds0 = blocks[1].src_nodes.clone()
                stream.synchronize()
                # (b) against the host sampler, bit for bit
                h_top = gnc.sample_block_host(ptr_np, idx_np, seeds_np, fanout, seed=2, return_eid=True)
                h_low = gnc.sample_block_host(ptr_np, idx_np, h_top.src_nodes, fanout, seed=1, return_eid=True)
                for b, h in zip(blocks, (h_low, h_top)):
                    for f in ("ptr", "idx", "src_nodes", "eid"):
                        assert np.array_equal(getattr(b, f).cpu().numpy(), getattr(h, f)), (name, batch, fanout, f)
                with torch.cuda.stream(stream):
                    t_low, t_top = torch_layers(ptrs, idxs, seeds, fanout)
                stream.synchronize()
                check_torch_block(ptr_np, idx_np, seeds_np, fanout, t_top)
                check_torch_block(ptr_np, idx_np, t_top[3].cpu().numpy().astype(np.int64), fanout, t_low)

                def arm_global():
                    sampler.sample(seeds, fanout, seed=2, relabel=False)
                    sampler.sample(seeds0, fanout, seed=1, relabel=False)

                def arm_host():
                    top = gnc.sample_block_host(ptr_np, idx_np, seeds_np, fanout, seed=2, return_eid=True)
                    gnc.sample_block_host(ptr_np, idx_np, top.src_nodes, fanout, seed=1, return_eid=True)

                arms = {"global": arm_global,
                        "relabel": lambda: sampler.sample_layers(seeds, (fanout, fanout), seed=1, return_eid=True),
                        "torch": lambda: torch_layers(ptrs, idxs, seeds, fanout)}
                for fn in arms.values():
                    time_round(fn, 2)
                times = {arm: [] for arm in list(arms) + ["host"]}
                for _ in range(args.rounds):
                    for arm, fn in arms.items():
                        times[arm].append(time_round(fn, args.calls))
                    t0 = time.perf_counter()
                    for _ in range(args.host_calls):
                        arm_host()
                    times["host"].append((time.perf_counter() - t0) * 1e6 / args.host_calls)
                # (e) a per-batch handle on the input-layer block
                blk = blocks[0]
                x = torch.randn((blk.num_src, 128), device=dev)
                y = torch.empty((blk.num_dst, 128), device=dev)
                first, steady = [], []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    agg = blk.gcn()
                    agg.run(x, y, 512, 0, reduce="mean")
                    torch.cuda.synchronize()
                    first.append((time.perf_counter() - t0) * 1e6)
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        agg.run(x, y, 512, 0, reduce="mean")
                    torch.cuda.synchronize()
                    steady.append((time.perf_counter() - t0) * 1e6 / args.calls)
                    agg.close()
                med = {arm: statistics.median(t) for arm, t in times.items()}
                rec = dict(input="%s-shaped two-layer sampling" % name, library=args.label, V=V, E=E, max_degree=int(np.diff(ptr_np).max()), batch=n, fanout=fanout, rounds=args.rounds,
                           calls=args.calls, host_calls=args.host_calls, host_threads=int(os.environ["OMP_NUM_THREADS"]),
                           edges=[b.num_edges for b in blocks], src_rows=[b.num_src for b in blocks],
                           torch_over_relabel=med["torch"] / med["relabel"], host_over_relabel=med["host"] / med["relabel"],
                           relabel_beats_torch_by_more_than_the_spread=bool(max(times["relabel"]) < min(times["torch"])),
                           handle_create_first_run_us=statistics.median(first), handle_steady_run_us=statistics.median(steady))
                for arm, t in times.items():
                    rec[arm + "_us"] = med[arm]
                    rec[arm + "_min_max_us"] = [min(t), max(t)]
                print(json.dumps(rec), flush=True)
        sampler.close()


if __name__ == "__main__":
    main()
