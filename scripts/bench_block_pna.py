#!/usr/bin/env python3
"""The block PNA layer (Block.pna; gnnagg_block_pna_run) against the layer a user writes today: the input-layer block of a two-layer
batch of the arxiv- and products-shaped graphs, 1 024 / 8 192 seeds, fanout 10 / 25, mean / min / max / std, self term + bias + ReLU.
Shapes: feat 128 -> 64 as fp32 with all three scalers and as bf16 with identity alone (the largest bf16 shape whose weight image fits the
LDS), and feat 64 -> 64 with all three scalers in both types.  Arms:

    f   the fused call: one launch                                                                    (blk.pna(..., fused=True))
    c   the composition: x[src_nodes], blk.gcn(val), run_multi, close, cat, matmul_NN, bias, ReLU        (blk.pna(..., fused=False))

The block is sampled once outside the timing.  The arms alternate inside every round on a non-null stream; a round times `--calls`
back-to-back calls of one arm (wall clock around a stream synchronisation); the figure of an arm is the median over `--rounds` rounds, with
the minimum and maximum of a round.  (f) is checked against (c) on every shape: fp32 bit for bit (a sampled row has at most `fanout`
edges), bf16 inside 2^-5 of the largest output ((c) rounds the scaled M and out to bf16; (f) the unscaled aggregates and out).  One JSON
line per (graph, batch, fanout, shape); nothing is asserted about speed.

    python scripts/bench_block_pna.py [--rounds 9] [--calls 20] [--datasets arxiv,products] [--batches 1024,8192] [--fanouts 10,25]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AGGRS = ("mean", "min", "max", "std")
ALL_SCALERS = ("identity", "amplification", "attenuation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--datasets", default="arxiv,products")
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--fanouts", default="10,25")
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_block_pna.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    f32, b16 = torch.float32, torch.bfloat16
    shapes = [(128, 64, f32, "fp32", ALL_SCALERS), (128, 64, b16, "bf16->bf16", ("identity",)), (64, 64, f32, "fp32", ALL_SCALERS),
              (64, 64, b16, "bf16->bf16", ALL_SCALERS)]

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
        delta = gnc.pna_delta(ptrs)
        sampler = gnc.NeighborSampler(ptrs, idxs)
        x128 = torch.randn((V, 128), device=dev)
        for batch in (int(b) for b in args.batches.split(",")):
            n = min(batch, V)
            seeds = torch.from_numpy(np.random.default_rng(11).choice(V, n, replace=False).astype(np.int32)).to(dev)
            for fanout in (int(f) for f in args.fanouts.split(",")):
                with torch.cuda.stream(stream):
                    blk = sampler.sample_layers(seeds, (fanout, fanout), seed=1)[0]
                stream.synchronize()
                for F, N, dt, tag, scalers in shapes:
                    assert gnc.block_pna_supported(F, N, len(AGGRS), len(scalers), dt), (F, N, tag, scalers)
                    x = x128[:, :F].contiguous().to(dt)
                    K = len(scalers) * len(AGGRS) * F
                    w, ws = (torch.randn((K, N), device=dev) / K ** 0.5).to(dt), (torch.randn((F, N), device=dev) / F ** 0.5).to(dt)
                    b = torch.randn(N, device=dev)
                    out = torch.empty((blk.num_dst, N), device=dev, dtype=dt)
                    kw = dict(w_self=ws, bias=b, aggrs=AGGRS, scalers=scalers, delta=delta, relu=True)
                    torch.cuda.synchronize()   # the operands were made on the default stream; the arms run on `stream`

                    def arm_f():
                        return blk.pna(x, w, out=out, fused=True, **kw)

                    def arm_c():
                        return blk.pna(x, w, fused=False, **kw)

                    with torch.cuda.stream(stream):
                        got, want = arm_f().clone(), arm_c()
                    stream.synchronize()
                    if dt == f32:
                        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, batch, fanout, F)
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
                               n_out=N, aggrs=len(AGGRS), scalers=len(scalers), rounds=args.rounds, calls=args.calls, num_dst=blk.num_dst,
                               num_src=blk.num_src, edges=blk.num_edges, c_over_f=med["c"] / med["f"],
                               f_beats_c_by_more_than_the_spread=bool(max(times["f"]) < min(times["c"])),
                               c_beats_f_by_more_than_the_spread=bool(max(times["c"]) < min(times["f"])), worst_abs_diff_f_c=worst)
                    for arm, t in times.items():
                        rec[arm + "_us"] = med[arm]
                        rec[arm + "_min_max_us"] = [min(t), max(t)]
                    print(json.dumps(rec), flush=True)
        sampler.close()


if __name__ == "__main__":
    main()
