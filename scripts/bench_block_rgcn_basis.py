#!/usr/bin/env python3
"""The basis-decomposed block R-GCN layer (Block.rgcn_basis; gnnagg_block_rgcn_basis_run) against the route a caller had before it, with
the protocol of bench_block_rgcn.py: the input-layer block of a two-layer batch of the arxiv- and products-shaped graphs, 1 024 / 8 192
seeds, fanout 10 / 25, random types, R in {8, 46, 266} relations, B in {2, 8, 30} bases, feat -> n_out in {128 -> 64, 64 -> 64, 64 -> 16},
mean + bias + ReLU, fp32 and bf16 -> bf16.  Arms:

    n   the fused call: one launch                                                               (blk.rgcn_basis(..., fused=True))
    c   w_rel = einsum(comp, bases) in x's dtype, then Block.rgcn with its own fused=None: its kernel
        where R fits its LDS, else one filtered sub-block and one aggregation per relation and a GEMM  (blk.rgcn_basis(..., fused=False))

The block and its types are made once outside the timing.  The arms alternate inside every round on a non-null stream; a round times
`--calls` back-to-back calls of one arm (wall clock around a stream synchronisation); the figure of an arm is the median over `--rounds`
rounds, with the minimum and maximum of a round.  The largest |n - c| is recorded beside the largest |c| on every shape (the two round
differently: (c) rounds w_rel; tests/test_gpu_block_rgcn_basis.py is the judge).  A shape outside gnnagg_block_rgcn_basis_supported is recorded as such and not timed.  One JSON line
per (graph, batch, fanout, R, B, feat, n_out, operand types); nothing is asserted about speed.

    python scripts/bench_block_rgcn_basis.py [--rounds 9] [--calls 20] [--datasets arxiv,products] [--batches 1024,8192] [--fanouts 10,25]
                                             [--relations 8,46,266] [--bases 2,8,30] [--shapes 128x64,64x64,64x16]"""
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
    ap.add_argument("--relations", default="8,46,266")
    ap.add_argument("--bases", default="2,8,30")
    ap.add_argument("--shapes", default="128x64,64x64,64x16")
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_block_rgcn_basis.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    ints = lambda s: [int(v) for v in s.split(",")]
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]

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
        x_all = torch.randn((V, max(s[0] for s in shapes)), device=dev)
        for batch in ints(args.batches):
            n = min(batch, V)
            seeds = torch.from_numpy(np.random.default_rng(11).choice(V, n, replace=False).astype(np.int32)).to(dev)
            for fanout in ints(args.fanouts):
                with torch.cuda.stream(stream):
                    blk = sampler.sample_layers(seeds, (fanout, fanout), seed=1)[0]
                stream.synchronize()
                for R in ints(args.relations):
                    etype = torch.from_numpy(np.random.default_rng(R).integers(0, R, blk.num_edges).astype(np.int32)).to(dev)
                    for B in ints(args.bases):
                        for (F, n_out) in shapes:
                            for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16->bf16")):
                                rec = dict(input="%s-shaped input-layer block" % name, library=args.label, V=V, E=E, batch=n, fanout=fanout,
                                           types=tag, feat=F, n_out=n_out, relations=R, bases=B, rounds=args.rounds, calls=args.calls,
                                           num_dst=blk.num_dst, num_src=blk.num_src, edges=blk.num_edges,
                                           c_is="einsum + " + ("k_block_rgcn" if gnc.block_rgcn_supported(F, n_out, R, dt) else "per-relation composition"))
                                if not gnc.block_rgcn_basis_supported(F, n_out, R, B, dt):
                                    print(json.dumps(dict(rec, supported=False)), flush=True)
                                    continue
                                x = x_all[:, :F].contiguous().to(dt)
                                ws = (torch.randn((F, n_out), device=dev) / F ** 0.5).to(dt)
                                bases = (torch.randn((B, F, n_out), device=dev) / F ** 0.5).to(dt)
                                comp = torch.randn((R, B), device=dev) / B ** 0.5
                                bias = torch.randn(n_out, device=dev)
                                out = torch.empty((blk.num_dst, n_out), device=dev, dtype=dt)
                                torch.cuda.synchronize()   # the operands were made on the default stream; the arms run on `stream`
                                kw = dict(w_self=ws, bias=bias, reduce="mean", relu=True)

                                def arm_n():
                                    return blk.rgcn_basis(x, bases, comp, etype, out=out, fused=True, **kw)

                                def arm_c():
                                    return blk.rgcn_basis(x, bases, comp, etype, fused=False, **kw)

                                with torch.cuda.stream(stream):
                                    got, want = arm_n().clone(), arm_c()
                                stream.synchronize()
                                where = (name, batch, fanout, R, B, F, n_out, tag)
                                assert torch.isfinite(got).all().item() and torch.isfinite(want).all().item(), where
                                worst = float((got.double() - want.double()).abs().max())
                                rec.update(largest_abs_c=float(want.double().abs().max()))   # (tests/test_gpu_block_rgcn_basis.py is the judge)
                                arms = {"n": arm_n, "c": arm_c}
                                for fn in arms.values():
                                    time_round(fn, 2)
                                times = {arm: [] for arm in arms}
                                for _ in range(args.rounds):
                                    for arm, fn in arms.items():
                                        times[arm].append(time_round(fn, args.calls))
                                med = {arm: statistics.median(t) for arm, t in times.items()}
                                rec.update(supported=True, c_over_n=med["c"] / med["n"],
                                           n_beats_c_by_more_than_the_spread=bool(max(times["n"]) < min(times["c"])),
                                           c_beats_n_by_more_than_the_spread=bool(max(times["c"]) < min(times["n"])), worst_abs_diff_n_c=worst)
                                for arm, t in times.items():
                                    rec[arm + "_us"] = med[arm]
                                    rec[arm + "_min_max_us"] = [min(t), max(t)]
                                print(json.dumps(rec), flush=True)
        sampler.close()


if __name__ == "__main__":
    main()
