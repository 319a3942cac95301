#!/usr/bin/env python3
"""Block aggregation (Block.aggregate; gnnagg_block_gcn_run) against what a mini-batch pays without it: the input-layer block of a
two-layer batch of the arxiv- and products-shaped graphs, 1 024 / 8 192 seeds, fanout 10 / 25, F = 128, mean, fp32 and bf16 -> bf16.  Arms:

    n   the new call on the FULL x, read through src_nodes                                   (no gather, no handle)
    g   the new call on an already gathered x (gathered=True)                                (what the map costs: n / g)
    b   what a user does today: x[src_nodes] + Aggregator_GCN create + run + close           (rows mode; bf16: "balanced", the typed call
                                                                                              refuses the rows mode)
    s0  x[src_nodes] + the steady rows-mode run of a handle made beforehand (fp32 only)      (the floor a plan buys: n / s)
    sb  x[src_nodes] + the steady "balanced" run of a handle made beforehand

The block is sampled once outside the timing.  The arms alternate inside every round on a non-null stream; a round times `--calls`
back-to-back calls of one arm (wall clock around a stream synchronisation); the figure of an arm is the median over `--rounds` rounds, with
the minimum and maximum of a round.  Beside the times: the byte model E F esize + 8 E + 4 (num_dst + 1) in, num_dst F ysize out, and what
it gives at arm n's time.  (n) is checked against (b) bit for bit (fp32) on every shape.  One JSON line per (graph, batch, fanout, types);
nothing is asserted about speed.

    python scripts/bench_block_run.py [--rounds 9] [--calls 20] [--datasets arxiv,products] [--batches 1024,8192] [--fanouts 10,25]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--datasets", default="arxiv,products")
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--fanouts", default="10,25")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_block_run.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    F = args.feat

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
        sampler = gnc.NeighborSampler(ptrs, idxs)
        x32 = torch.randn((V, F), device=dev)
        for batch in (int(b) for b in args.batches.split(",")):
            n = min(batch, V)
            seeds = torch.from_numpy(np.random.default_rng(11).choice(V, n, replace=False).astype(np.int32)).to(dev)
            for fanout in (int(f) for f in args.fanouts.split(",")):
                with torch.cuda.stream(stream):
                    blk = sampler.sample_layers(seeds, (fanout, fanout), seed=1)[0]
                    src = blk.src_nodes.long()
                stream.synchronize()
                for xdt, ydt, tag in ((torch.float32, torch.float32, "fp32"), (torch.bfloat16, torch.bfloat16, "bf16->bf16")):
                    x = x32 if xdt == torch.float32 else x32.to(xdt)
                    x_src = x[src].contiguous()
                    y = torch.empty((blk.num_dst, F), device=dev, dtype=ydt)
                    y2 = torch.empty_like(y)
                    rows_ok = xdt == torch.float32
                    mode_b = 0 if rows_ok else "balanced"

                    def arm_b():
                        h = x[src]
                        agg = blk.gcn()
                        agg.run(h, y2, 512, mode_b, reduce="mean")
                        agg.close()

                    with torch.cuda.stream(stream):
                        steady = blk.gcn()
                        if rows_ok:
                            steady.run(x_src, y2, 512, 0, reduce="mean")
                        steady.run(x_src, y2, 512, "balanced", reduce="mean")
                        blk.aggregate(x, reduce="mean", out=y)
                        arm_b()
                    stream.synchronize()
                    if rows_ok:
                        assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), (name, batch, fanout)
                    arms = {"n": lambda: blk.aggregate(x, reduce="mean", out=y),
                            "g": lambda: blk.aggregate(x_src, reduce="mean", gathered=True, out=y),
                            "b": arm_b,
                            "sb": lambda: steady.run(x[src], y2, 512, "balanced", reduce="mean")}
                    if rows_ok:
                        arms["s0"] = lambda: steady.run(x[src], y2, 512, 0, reduce="mean")
                    for fn in arms.values():
                        time_round(fn, 2)
                    times = {arm: [] for arm in arms}
                    for _ in range(args.rounds):
                        for arm, fn in arms.items():
                            times[arm].append(time_round(fn, args.calls))
                    with torch.cuda.stream(stream):
                        steady.close()
                    med = {arm: statistics.median(t) for arm, t in times.items()}
                    esize = x.element_size()
                    bytes_in = blk.num_edges * F * esize + 8 * blk.num_edges + 4 * (blk.num_dst + 1)
                    bytes_out = blk.num_dst * F * y.element_size()
                    s_best = min(med[a] for a in ("s0", "sb") if a in med)
                    rec = dict(input="%s-shaped input-layer block" % name, library=args.label, V=V, E=E, batch=n, fanout=fanout, types=tag, feat=F,
                               rounds=args.rounds, calls=args.calls, num_dst=blk.num_dst, num_src=blk.num_src, edges=blk.num_edges,
                               model_bytes_in=bytes_in, model_bytes_out=bytes_out, model_GBps_at_n=(bytes_in + bytes_out) / med["n"] / 1e3,
                               b_over_n=med["b"] / med["n"], n_over_s=med["n"] / s_best, n_over_g=med["n"] / med["g"],
                               n_beats_b_by_more_than_the_spread=bool(max(times["n"]) < min(times["b"])))
                    for arm, t in times.items():
                        rec[arm + "_us"] = med[arm]
                        rec[arm + "_min_max_us"] = [min(t), max(t)]
                    print(json.dumps(rec), flush=True)
        sampler.close()


if __name__ == "__main__":
    main()
