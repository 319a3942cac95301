#!/usr/bin/env python3
"""The block GIN layer (Block.gin; gnnagg_block_gin_run) against the layer a user writes today: the input-layer block of a two-layer
batch of the arxiv- and products-shaped graphs, 1 024 / 8 192 seeds, fanout 10 / 25, feat 128 -> hidden 128 -> n_out 64, sum + both biases
+ final ReLU, fp32 and bf16 -> bf16.  Arms:

    f   the fused call: one launch                                                                    (blk.gin(..., fused=True))
    c   the composition: blk.aggregate(return_dst=True), a product, a sum, two matmul_NN, biases, ReLUs  (blk.gin(..., fused=False))

The block is sampled once outside the timing.  The arms alternate inside every round on a non-null stream; a round times `--calls`
back-to-back calls of one arm (wall clock around a stream synchronisation); the figure of an arm is the median over `--rounds` rounds, with
the minimum and maximum of a round.  (f) is checked against (c) on every shape: fp32 bit for bit, bf16 inside 2^-5 of the largest output
((c) rounds y, the product, h, z and out to bf16; (f) h, z and out).  One JSON line per (graph, batch, fanout, types); nothing is asserted
about speed.

    python scripts/bench_block_gin.py [--rounds 9] [--calls 20] [--datasets arxiv,products] [--batches 1024,8192] [--fanouts 10,25]"""
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
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--n-out", type=int, default=64)
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_block_gin.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    F, H, N = args.feat, args.hidden, args.n_out

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
                stream.synchronize()
                for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16->bf16")):
                    x = x32 if dt == torch.float32 else x32.to(dt)
                    w1, w2 = (torch.randn((F, H), device=dev) / F ** 0.5).to(dt), (torch.randn((H, N), device=dev) / H ** 0.5).to(dt)
                    b1, b2 = torch.randn(H, device=dev), torch.randn(N, device=dev)
                    out = torch.empty((blk.num_dst, N), device=dev, dtype=dt)
                    kw = dict(b1=b1, b2=b2, eps=0.25, reduce="sum", relu=True)
                    torch.cuda.synchronize()   # the operands were made on the default stream; the arms run on `stream`

                    def arm_f():
                        return blk.gin(x, w1, w2, out=out, fused=True, **kw)

                    def arm_c():
                        return blk.gin(x, w1, w2, fused=False, **kw)

                    with torch.cuda.stream(stream):
                        got, want = arm_f().clone(), arm_c()
                    stream.synchronize()
                    if dt == torch.float32:
                        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, batch, fanout)
                    assert torch.isfinite(got).all().item() and torch.isfinite(want).all().item(), (name, batch, fanout, tag)
                    worst = float((got.double() - want.double()).abs().max())
                    assert worst <= 2.0 ** -5 * float(want.double().abs().max()), (name, batch, fanout, tag, worst)
                    arms = {"f": arm_f, "c": arm_c}
                    for fn in arms.values():
                        time_round(fn, 2)
                    times = {arm: [] for arm in arms}
                    for _ in range(args.rounds):
                        for arm, fn in arms.items():
                            times[arm].append(time_round(fn, args.calls))
                    med = {arm: statistics.median(t) for arm, t in times.items()}
                    rec = dict(input="%s-shaped input-layer block" % name, library=args.label, V=V, E=E, batch=n, fanout=fanout, types=tag, feat=F,
                               hidden=H, n_out=N, rounds=args.rounds, calls=args.calls, num_dst=blk.num_dst, num_src=blk.num_src,
                               edges=blk.num_edges, c_over_f=med["c"] / med["f"],
                               f_beats_c_by_more_than_the_spread=bool(max(times["f"]) < min(times["c"])),
                               c_beats_f_by_more_than_the_spread=bool(max(times["c"]) < min(times["f"])), worst_abs_diff_f_c=worst)
                    for arm, t in times.items():
                        rec[arm + "_us"] = med[arm]
                        rec[arm + "_min_max_us"] = [min(t), max(t)]
                    print(json.dumps(rec), flush=True)
        sampler.close()


if __name__ == "__main__":
    main()
