#!/usr/bin/env python3
"""The block R-GCN layer (Block.rgcn; gnnagg_block_rgcn_run) against the layer a user writes today, on the shapes of bench_block_sage.py:
the input-layer block of a two-layer batch of the arxiv- and products-shaped graphs, 1 024 / 8 192 seeds, fanout 10 / 25, feat = 128,
n_out = 64, R = 4 and 8 relations, types random and types sorted within rows, mean + bias + ReLU, fp32 and bf16 -> bf16.  Arms:

    f   the fused call: one launch                                                                  (blk.rgcn(..., fused=True))
    c   the composition: per relation a filtered sub-block built with torch ops and blk.aggregate,
        then cat, one matmul_NN, bias, ReLU                                                         (blk.rgcn(..., fused=False))

The block and its types are made once outside the timing.  The arms alternate inside every round on a non-null stream; a round times
`--calls` back-to-back calls of one arm (wall clock around a stream synchronisation); the figure of an arm is the median over `--rounds`
rounds, with the minimum and maximum of a round.  (f) is checked against (c) on every shape: fp32 bit for bit, bf16 inside 2^-6 of the
largest output.  A shape outside gnnagg_block_rgcn_supported is recorded as such and not timed.  One JSON line per (graph, batch, fanout,
R, order of types, operand types); nothing is asserted about speed.

    python scripts/bench_block_rgcn.py [--rounds 9] [--calls 20] [--datasets arxiv,products] [--batches 1024,8192] [--fanouts 10,25]"""
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
    ap.add_argument("--relations", default="4,8")
    ap.add_argument("--n-out", type=int, default=64)
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_block_rgcn.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    F, n_out = args.feat, args.n_out

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
                ptr = blk.ptr.cpu().numpy().astype(np.int64)
                row = np.repeat(np.arange(blk.num_dst), np.diff(ptr))
                for R in (int(r) for r in args.relations.split(",")):
                    t_rand = np.random.default_rng(R).integers(0, R, blk.num_edges)
                    for order, t_np in (("random", t_rand), ("sorted within rows", t_rand[np.lexsort((t_rand, row))])):
                        etype = torch.from_numpy(t_np.astype(np.int32)).to(dev)
                        for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16->bf16")):
                            rec = dict(input="%s-shaped input-layer block" % name, library=args.label, V=V, E=E, batch=n, fanout=fanout, types=tag,
                                       feat=F, n_out=n_out, relations=R, etype_order=order, rounds=args.rounds, calls=args.calls,
                                       num_dst=blk.num_dst, num_src=blk.num_src, edges=blk.num_edges)
                            if not gnc.block_rgcn_supported(F, n_out, R, dt):
                                print(json.dumps(dict(rec, supported=False)), flush=True)
                                continue
                            x = x32 if dt == torch.float32 else x32.to(dt)
                            ws = (torch.randn((F, n_out), device=dev) / F ** 0.5).to(dt)
                            wr = (torch.randn((R, F, n_out), device=dev) / F ** 0.5).to(dt)
                            bias = torch.randn(n_out, device=dev)
                            out = torch.empty((blk.num_dst, n_out), device=dev, dtype=dt)
                            torch.cuda.synchronize()   # the operands were made on the default stream; the arms run on `stream`
                            kw = dict(w_self=ws, bias=bias, reduce="mean", relu=True)

                            def arm_f():
                                return blk.rgcn(x, wr, etype, out=out, fused=True, **kw)

                            def arm_c():
                                return blk.rgcn(x, wr, etype, fused=False, **kw)

                            with torch.cuda.stream(stream):
                                got, want = arm_f().clone(), arm_c()
                            stream.synchronize()
                            if dt == torch.float32:
                                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, batch, fanout, R, order)
                            assert torch.isfinite(got).all().item() and torch.isfinite(want).all().item(), (name, batch, fanout, R, order, tag)
                            worst = float((got.double() - want.double()).abs().max())
                            assert worst <= 2.0 ** -6 * float(want.double().abs().max()), (name, batch, fanout, R, order, tag, worst)
                            arms = {"f": arm_f, "c": arm_c}
                            for fn in arms.values():
                                time_round(fn, 2)
                            times = {arm: [] for arm in arms}
                            for _ in range(args.rounds):
                                for arm, fn in arms.items():
                                    times[arm].append(time_round(fn, args.calls))
                            med = {arm: statistics.median(t) for arm, t in times.items()}
                            rec.update(supported=True, c_over_f=med["c"] / med["f"],
                                       f_beats_c_by_more_than_the_spread=bool(max(times["f"]) < min(times["c"])),
                                       c_beats_f_by_more_than_the_spread=bool(max(times["c"]) < min(times["f"])), worst_abs_diff_f_c=worst)
                            for arm, t in times.items():
                                rec[arm + "_us"] = med[arm]
                                rec[arm + "_min_max_us"] = [min(t), max(t)]
                            print(json.dumps(rec), flush=True)
        sampler.close()


if __name__ == "__main__":
    main()
