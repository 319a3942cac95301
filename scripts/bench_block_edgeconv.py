#!/usr/bin/env python3
"""Block.edgeconv (gnnagg_block_edgeconv_run) against what a user writes today, on the input-layer block of a two-layer sampled batch of
the arxiv- and products-shaped graphs, 1 024 / 8 192 seeds, fanout 10 / 25, F = 3 and 64, hidden = n_out = 64, fp32 and bf16, max and
mean.  Arms:

    f   the fused call: one launch                                          (blk.edgeconv(x, w1, w2, b1, b2, fused=True))
    c   the composition: two index calls, a difference, cat, two matmul_NN, biases, ReLU and Block.aggregate over the [E, n_out]
        messages                                                            (fused=False)

The block is sampled once outside the timing.  The arms alternate inside every round on a non-null stream; a round times `--calls`
back-to-back calls of one arm (wall clock around a stream synchronisation); the figure of an arm is the median over `--rounds` rounds,
with the minimum and maximum of a round.  (f) is checked against (c) on every shape: fp32 max bit for bit, everything else inside 2^-5 of
the largest output.  One JSON line per shape; nothing is asserted about speed.

    python scripts/bench_block_edgeconv.py [--rounds 7] [--calls 10] [--datasets arxiv,products] [--batches 1024,8192] [--fanouts 10,25]
                                           [--feats 3,64] [--hidden 64] [--n-out 64] [--combines diff] [--reduces max,mean] [--label main]"""
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--datasets", default="arxiv,products")
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--fanouts", default="10,25")
    ap.add_argument("--feats", default="3,64")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--n-out", type=int, default=64)
    ap.add_argument("--combines", default="diff")
    ap.add_argument("--reduces", default="max,mean")
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_block_edgeconv.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    H, N = args.hidden, args.n_out

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
        V = ptrs.numel() - 1
        sampler = gnc.NeighborSampler(ptrs, idxs)
        for batch in (int(b) for b in args.batches.split(",")):
            n = min(batch, V)
            seeds = torch.from_numpy(np.random.default_rng(11).choice(V, n, replace=False).astype(np.int32)).to(dev)
            for fanout in (int(f) for f in args.fanouts.split(",")):
                with torch.cuda.stream(stream):
                    blk = sampler.sample_layers(seeds, (fanout, fanout), seed=1)[0]
                    max_deg = int((blk.ptr[1:] - blk.ptr[:-1]).max().item())
                stream.synchronize()
                for F in (int(f) for f in args.feats.split(",")):
                    x32 = torch.randn((V, F), device=dev)
                    for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
                        x = x32.to(dt)
                        w1, w2 = (torch.randn((2 * F, H), device=dev) / (2 * F) ** 0.5).to(dt), (torch.randn((H, N), device=dev) / H ** 0.5).to(dt)
                        b1, b2 = torch.randn(H, device=dev), torch.randn(N, device=dev)
                        out = torch.empty((blk.num_dst, N), device=dev, dtype=dt)
                        for combine in args.combines.split(","):
                            for reduce in args.reduces.split(","):
                                base = dict(input="%s-shaped input-layer block" % name, library=args.label, batch=n, fanout=fanout, types=tag,
                                            feat=F, hidden=H, n_out=N, combine=combine, reduce=reduce, rounds=args.rounds, calls=args.calls,
                                            num_dst=blk.num_dst, num_src=blk.num_src, edges=blk.num_edges, max_deg=max_deg)
                                if not gnc.block_edgeconv_supported(combine, F, H, N, dt):
                                    print(json.dumps(dict(base, supported=False)), flush=True)
                                    continue
                                kw = dict(b1=b1, b2=b2, combine=combine, reduce=reduce, relu=True)
                                arms = {"f": lambda: blk.edgeconv(x, w1, w2, out=out, fused=True, **kw),
                                        "c": lambda: blk.edgeconv(x, w1, w2, fused=False, **kw)}
                                torch.cuda.synchronize()   # the operands were made on the default stream; the arms run on `stream`
                                with torch.cuda.stream(stream):
                                    got, want = arms["f"]().clone(), arms["c"]()
                                stream.synchronize()
                                if dt == torch.float32 and reduce == "max":
                                    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, batch, fanout, F, combine)
                                worst = float((got.double() - want.double()).abs().max())
                                assert torch.isfinite(got).all().item() and worst <= 2.0 ** -5 * float(want.double().abs().max()), (name, tag, F, worst)
                                for fn in arms.values():
                                    time_round(fn, 2)
                                times = {arm: [] for arm in arms}
                                for _ in range(args.rounds):
                                    for arm, fn in arms.items():
                                        times[arm].append(time_round(fn, args.calls))
                                rec = dict(base, worst_abs_diff_f_c=worst, c_over_f=statistics.median(times["c"]) / statistics.median(times["f"]),
                                           f_beats_c_by_more_than_the_spread=bool(max(times["f"]) < min(times["c"])),
                                           c_beats_f_by_more_than_the_spread=bool(max(times["c"]) < min(times["f"])))
                                for arm, t in times.items():
                                    rec[arm + "_us"] = statistics.median(t)
                                    rec[arm + "_min_max_us"] = [min(t), max(t)]
                                print(json.dumps(rec), flush=True)
        sampler.close()


if __name__ == "__main__":
    main()
