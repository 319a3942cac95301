#!/usr/bin/env python3
"""Block attention (Block.attend; gnnagg_block_attn_run) against what a mini-batch pays without it: the input-layer block of a two-layer
batch of the arxiv- and products-shaped graphs, 1 024 / 8 192 seeds, fanout 10 / 25, F = 128 with 1 and 4 heads, fp32 and bf16, dot-product
and GATv2; on the arxiv-shaped graph additionally with per-edge feature rows kept per edge of the FULL graph (edge=1).  Arms:

    a   the new call on the operands in place: q / k / v per row of the full graph, read through src_nodes (edge rows through eid)
    b   what a user does today: q[src], k[src], v[src] (ef[eid]) + Aggregator_GAT create + run_dot / run_v2 + close
    c   the same gathers + the steady run of a handle made beforehand (the floor a plan buys)

The block is sampled once outside the timing.  The arms alternate inside every round on a non-null stream; a round times `--calls`
back-to-back calls of one arm (wall clock around a stream synchronisation); the figure of an arm is the median over `--rounds` rounds, with
the minimum and maximum of a round.  (a) is checked against (c) bit for bit on every shape whose rows hold at most 128 edges.  One JSON line
per (graph, batch, fanout, kind, heads, types, edge); nothing is asserted about speed.

    python scripts/bench_block_attn.py [--rounds 9] [--calls 20] [--datasets arxiv,products] [--batches 1024,8192] [--fanouts 10,25]"""
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
    ap.add_argument("--heads", default="1,4")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--edge-datasets", default="arxiv", help="the graphs that also run with full-graph edge rows ([E, F] must fit)")
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_block_attn.py measures on the GPU only"
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
        qkv32 = torch.randn((V, 3 * F), device=dev)
        for batch in (int(b) for b in args.batches.split(",")):
            n = min(batch, V)
            seeds = torch.from_numpy(np.random.default_rng(11).choice(V, n, replace=False).astype(np.int32)).to(dev)
            for fanout in (int(f) for f in args.fanouts.split(",")):
                with torch.cuda.stream(stream):
                    blk = sampler.sample_layers(seeds, (fanout, fanout), seed=1, return_eid=True)[0]
                    src, eid = blk.src_nodes.long(), blk.eid.long()
                    max_deg = int((blk.ptr[1:] - blk.ptr[:-1]).max().item())
                stream.synchronize()
                for xdt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
                    qkv = qkv32 if xdt == torch.float32 else qkv32.to(xdt)
                    q, k, v = qkv[:, :F], qkv[:, F:2 * F], qkv[:, 2 * F:]        # column views of one projection, never copied
                    for with_edge in ((False, True) if name in args.edge_datasets.split(",") else (False,)):
                        ef = torch.randn((E, F), device=dev, dtype=xdt) if with_edge else None
                        for kind in ("dot", "gatv2"):
                            for H in (int(h) for h in args.heads.split(",")):
                                if with_edge and H != 4:
                                    continue
                                a = torch.randn(F, device=dev) / 8
                                y = torch.empty((blk.num_dst, F), device=dev, dtype=xdt)
                                y2 = torch.empty_like(y)

                                def arm_a():
                                    if kind == "dot":
                                        blk.attend(q, k, v, heads=H, edge=ef, edge_full=with_edge, out=y)
                                    else:
                                        blk.attend(q, k, kind="gatv2", a=a, heads=H, edge=ef, edge_full=with_edge, out=y)

                                def run(agg):
                                    e = ef[eid] if with_edge else None
                                    if kind == "dot":
                                        agg.run_dot(q[src], k[src], v[src], y2, heads=H, edge=e)
                                    else:
                                        agg.run_v2(k[src], q[src], a, y2, heads=H, edge=e)

                                def arm_b():
                                    agg = blk.gat()
                                    run(agg)
                                    agg.close()

                                torch.cuda.synchronize()   # the operands were made on the default stream: done before the timing stream reads them
                                with torch.cuda.stream(stream):
                                    steady = blk.gat()
                                    run(steady)
                                    arm_a()
                                stream.synchronize()
                                bits = torch.int32 if xdt == torch.float32 else torch.int16
                                same = bool(torch.equal(y.view(bits), y2.view(bits)))
                                assert same or max_deg > 128, (name, batch, fanout, kind, H, tag, with_edge, int((y.view(bits) != y2.view(bits)).sum()))
                                arms = {"a": arm_a, "b": arm_b, "c": lambda: run(steady)}
                                for fn in arms.values():
                                    time_round(fn, 2)
                                times = {arm: [] for arm in arms}
                                for _ in range(args.rounds):
                                    for arm, fn in arms.items():
                                        times[arm].append(time_round(fn, args.calls))
                                with torch.cuda.stream(stream):
                                    steady.close()
                                med = {arm: statistics.median(t) for arm, t in times.items()}
                                rec = dict(input="%s-shaped input-layer block" % name, library=args.label, V=V, E=E, batch=n, fanout=fanout,
                                           kind=kind, heads=H, types=tag, feat=F, edge=int(with_edge), rounds=args.rounds, calls=args.calls,
                                           num_dst=blk.num_dst, num_src=blk.num_src, edges=blk.num_edges, max_deg=max_deg, same_bits_as_handle=same,
                                           b_over_a=med["b"] / med["a"], c_over_a=med["c"] / med["a"],
                                           a_beats_b_by_more_than_the_spread=bool(max(times["a"]) < min(times["b"])),
                                           a_beats_c_by_more_than_the_spread=bool(max(times["a"]) < min(times["c"])))
                                for arm, t in times.items():
                                    rec[arm + "_us"] = med[arm]
                                    rec[arm + "_min_max_us"] = [min(t), max(t)]
                                print(json.dumps(rec), flush=True)
                        del ef
        sampler.close()


if __name__ == "__main__":
    main()
