#!/usr/bin/env python3
"""Weighted neighbour sampling (NeighborSampler(prob=); gnnagg_sampler_set_weights) against the unweighted sampler and against what a
caller composed before it, on the shapes and by the method of scripts/bench_sampling.py: two-layer mini-batches of the arxiv- and
products-shaped graphs, batches of 1 024 and 8 192 seeds and all rows, fanouts 10 and 25.  The weights are log-uniform over 12 binades
with 30 % zeros.  Arms:

    uniform     (u) sample_layers(seeds, (f, f), return_eid=True) on a sampler without weights
    weighted    (w) the same call on a sampler with the weights set
    torch       (c) the weighted blocks composed from torch ops: expand the seed rows, drop the edges without weight, keys -log(rand) / w,
                sort by (row, key), keep rank < fanout, torch.unique with inverse for the relabelling (sorted-id relabelling, rows not put
                back into CSR order -- both in its favour); checked to be a valid block of eligible edges
    host        (h) gnnagg_sample_block_host_weighted, the same two layers, on OMP_NUM_THREADS threads (16 unless the caller set it)
    set_weights gnnagg_sampler_set_weights alone (flags, one scan over the edges, the row differences, one synchronisation)
    hub         one block whose only seed is the row of the highest degree, uniform and weighted: what that row costs on its workgroup

(u), (w) and (c) alternate inside every round on a non-null stream; a round times `--calls` back-to-back calls of one arm (wall clock around
a stream synchronisation); the figure of an arm is the median over `--rounds` rounds, printed with the minimum and maximum of a round.  (w)
is checked against the host sampler bit for bit on every shape.  One JSON line per (graph, batch, fanout); nothing is asserted about speed.

    python scripts/bench_sampling_weighted.py [--rounds 9] [--calls 20] [--datasets arxiv,products] [--batches 1024,8192,all] [--fanouts 10,25]"""
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

    assert torch.cuda.is_available(), "bench_sampling_weighted.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()

    def torch_block(ptr, idx, w, seeds, fanout):
        sl = seeds.long()
        beg = ptr[sl].long()
        deg = ptr[sl + 1].long() - beg
        n = sl.numel()
        row = torch.repeat_interleave(torch.arange(n, device=dev), deg)
        start = torch.cumsum(deg, 0) - deg
        pos = beg[row] + (torch.arange(row.numel(), device=dev) - start[row])
        we = w[pos]
        ok = we > 0
        row, pos, we = row[ok], pos[ok], we[ok]
        dplus = torch.bincount(row, minlength=n)
        start = torch.cumsum(dplus, 0) - dplus
        total = row.numel()
        o1 = torch.argsort(-torch.log(torch.rand(total, device=dev)) / we)
        srow, o2 = torch.sort(row[o1], stable=True)
        keep = (torch.arange(total, device=dev) - start[srow]) < fanout
        eid, krow = pos[o1[o2]][keep], srow[keep]
        blk_ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(torch.clamp(dplus, max=fanout), 0)])
        src, inv = torch.unique(torch.cat([sl, idx[eid].long()]), return_inverse=True)
        return blk_ptr, inv[n:], eid, src, inv[:n], krow

    def torch_layers(ptr, idx, w, seeds, fanout):
        top = torch_block(ptr, idx, w, seeds, fanout)
        return torch_block(ptr, idx, w, top[3], fanout), top

    def check_torch_block(ptr_np, idx_np, w_np, seeds_np, fanout, blk):
        blk_ptr, bidx, eid, src, dst, krow = (t.cpu().numpy() for t in blk)
        before = np.concatenate([[0], np.cumsum(w_np > 0)])
        dplus = before[ptr_np[seeds_np + 1]] - before[ptr_np[seeds_np]]
        assert np.array_equal(np.diff(blk_ptr), np.minimum(dplus, fanout)) and blk_ptr[-1] == len(eid)
        assert np.array_equal(krow, np.repeat(np.arange(len(seeds_np)), np.diff(blk_ptr)))
        r = seeds_np[krow]
        assert ((eid >= ptr_np[r]) & (eid < ptr_np[r + 1])).all() and (w_np[eid] > 0).all()
        assert len(np.unique(eid)) == len(eid)
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
        rng = np.random.default_rng(12)
        w_np = np.exp2(rng.uniform(-6.0, 6.0, size=E)).astype(np.float32)
        w_np[rng.random(E) < 0.30] = 0.0
        w = torch.from_numpy(w_np).to(dev)
        uniform = gnc.NeighborSampler(ptrs, idxs)
        weighted = gnc.NeighborSampler(ptrs, idxs, prob=w)
        t_set = []
        with torch.cuda.stream(stream):
            for _ in range(args.rounds):
                stream.synchronize()
                t0 = time.perf_counter()
                weighted.set_prob(w)
                t_set.append((time.perf_counter() - t0) * 1e6)
        hub_row = int(np.argmax(np.diff(ptr_np)))
        hub_seed = torch.tensor([hub_row], dtype=torch.int32, device=dev)
        for batch in args.batches.split(","):
            n = V if batch == "all" else min(int(batch), V)
            seeds_np = (np.arange(V) if n == V else np.random.default_rng(11).choice(V, n, replace=False)).astype(np.int32)
            seeds = torch.from_numpy(seeds_np).to(dev)
            for fanout in (int(f) for f in args.fanouts.split(",")):
                with torch.cuda.stream(stream):
                    blocks = weighted.sample_layers(seeds, (fanout, fanout), seed=1, return_eid=True)
                    plain = uniform.sample_layers(seeds, (fanout, fanout), seed=1, return_eid=True)
                stream.synchronize()
                h_top = gnc.sample_block_host(ptr_np, idx_np, seeds_np, fanout, seed=2, return_eid=True, prob=w_np)
                h_low = gnc.sample_block_host(ptr_np, idx_np, h_top.src_nodes, fanout, seed=1, return_eid=True, prob=w_np)
                for b, h in zip(blocks, (h_low, h_top)):
                    for f in ("ptr", "idx", "src_nodes", "eid"):
                        assert np.array_equal(getattr(b, f).cpu().numpy(), getattr(h, f)), (name, batch, fanout, f)
                with torch.cuda.stream(stream):
                    t_low, t_top = torch_layers(ptrs, idxs, w, seeds, fanout)
                stream.synchronize()
                check_torch_block(ptr_np, idx_np, w_np, seeds_np, fanout, t_top)
                check_torch_block(ptr_np, idx_np, w_np, t_top[3].cpu().numpy().astype(np.int64), fanout, t_low)

                def arm_host():
                    top = gnc.sample_block_host(ptr_np, idx_np, seeds_np, fanout, seed=2, return_eid=True, prob=w_np)
                    gnc.sample_block_host(ptr_np, idx_np, top.src_nodes, fanout, seed=1, return_eid=True, prob=w_np)

                arms = {"uniform": lambda: uniform.sample_layers(seeds, (fanout, fanout), seed=1, return_eid=True),
                        "weighted": lambda: weighted.sample_layers(seeds, (fanout, fanout), seed=1, return_eid=True),
                        "torch": lambda: torch_layers(ptrs, idxs, w, seeds, fanout),
                        "hub_uniform": lambda: uniform.sample(hub_seed, fanout, seed=1, return_eid=True),
                        "hub_weighted": lambda: weighted.sample(hub_seed, fanout, seed=1, return_eid=True)}
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
                med = {arm: statistics.median(t) for arm, t in times.items()}
                rec = dict(input="%s-shaped two-layer weighted sampling" % name, library=args.label, V=V, E=E, max_degree=int(np.diff(ptr_np).max()),
                           batch=n, fanout=fanout, rounds=args.rounds, calls=args.calls, host_calls=args.host_calls,
                           host_threads=int(os.environ["OMP_NUM_THREADS"]), edges=[b.num_edges for b in blocks],
                           uniform_edges=[b.num_edges for b in plain], src_rows=[b.num_src for b in blocks],
                           weighted_over_uniform=med["weighted"] / med["uniform"], torch_over_weighted=med["torch"] / med["weighted"],
                           host_over_weighted=med["host"] / med["weighted"],
                           weighted_beats_torch_by_more_than_the_spread=bool(max(times["weighted"]) < min(times["torch"])),
                           set_weights_us=statistics.median(t_set), set_weights_min_max_us=[min(t_set), max(t_set)])
                for arm, t in times.items():
                    rec[arm + "_us"] = med[arm]
                    rec[arm + "_min_max_us"] = [min(t), max(t)]
                print(json.dumps(rec), flush=True)
        uniform.close()
        weighted.close()


if __name__ == "__main__":
    main()
