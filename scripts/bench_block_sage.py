#!/usr/bin/env python3
"""The block SAGE layer (Block.sage; gnnagg_block_sage_run) against the layer a user writes today: the input-layer block of a two-layer
batch of the arxiv- and products-shaped graphs, 1 024 / 8 192 seeds, fanout 10 / 25, feat = 128, n_out 64 / 128, mean + bias + ReLU, fp32
and bf16 -> bf16.  Arms:

    f   the fused call: one launch                                                           (blk.sage(..., fused=True))
    w   the chunked kernel for wide rows: one launch                                         (blk.sage(..., fused="wide"))
    c   the composition: blk.aggregate(return_dst=True), two matmul_NN, add, bias, ReLU      (the yardstick)

The block is sampled once outside the timing.  The arms alternate inside every round on a non-null stream; a round times `--calls`
back-to-back calls of one arm (wall clock around a stream synchronisation); the figure of an arm is the median over `--rounds` rounds, with
the minimum and maximum of a round.  (f) runs where F and n_out lie in its range (<= 256), (w) everywhere: --feat 512 / 602 / 1024 time
(w) against (c), --feat 128 all three.  (f) and (w) are checked against (c) on every shape: fp32 against the one-GEMM form of the composition bit for
bit, bf16 inside 2^-6 of the largest output (two roundings of y and of out apart).  One JSON line per (graph, batch, fanout, n_out,
types); nothing is asserted about speed.

    python scripts/bench_block_sage.py [--rounds 9] [--calls 20] [--datasets arxiv,products] [--batches 1024,8192] [--fanouts 10,25]"""
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
    ap.add_argument("--n-outs", default="64,128")
    ap.add_argument("--feat", type=int, default=128)
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_block_sage.py measures on the GPU only"
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
                stream.synchronize()
                for n_out in (int(v) for v in args.n_outs.split(",")):
                    for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16->bf16")):
                        x = x32 if dt == torch.float32 else x32.to(dt)
                        ws, wn = ((torch.randn((F, n_out), device=dev) / F ** 0.5).to(dt) for _ in range(2))
                        bias = torch.randn(n_out, device=dev)
                        out = torch.empty((blk.num_dst, n_out), device=dev, dtype=dt)
                        torch.cuda.synchronize()   # the operands were made on the default stream; the arms run on `stream`

                        def arm_f():
                            return blk.sage(x, wn, ws, bias, reduce="mean", relu=True, out=out, fused=True)

                        def arm_c():
                            y, x_dst = blk.aggregate(x, reduce="mean", return_dst=True)
                            return torch.relu(gnc.matmul_NN(x_dst, ws, out_dtype=torch.float32) + gnc.matmul_NN(y, wn, out_dtype=torch.float32)
                                              + bias).to(dt)

                        def arm_w():
                            return blk.sage(x, wn, ws, bias, reduce="mean", relu=True, out=out, fused="wide")

                        arms = {"f": arm_f} if gnc.block_sage_supported(F, n_out, dt) else {}
                        arms.update(w=arm_w, c=arm_c)
                        with torch.cuda.stream(stream):
                            want = arm_c()
                            one_gemm = blk.sage(x, wn, ws, bias, reduce="mean", relu=True, fused=False)
                        worst = {}
                        for arm in [a for a in arms if a != "c"]:
                            with torch.cuda.stream(stream):
                                got = arms[arm]().clone()
                            stream.synchronize()
                            if dt == torch.float32:
                                assert torch.equal(got.view(torch.int32), one_gemm.view(torch.int32)), (arm, name, batch, fanout, n_out)
                            assert torch.isfinite(got).all().item() and torch.isfinite(want).all().item(), (arm, name, batch, fanout, n_out, tag)
                            worst[arm] = float((got.double() - want.double()).abs().max())
                            assert worst[arm] <= 2.0 ** -6 * float(want.double().abs().max()), (arm, name, batch, fanout, n_out, tag, worst[arm])
                        for fn in arms.values():
                            time_round(fn, 2)
                        times = {arm: [] for arm in arms}
                        for _ in range(args.rounds):
                            for arm, fn in arms.items():
                                times[arm].append(time_round(fn, args.calls))
                        med = {arm: statistics.median(t) for arm, t in times.items()}
                        rec = dict(input="%s-shaped input-layer block" % name, library=args.label, V=V, E=E, batch=n, fanout=fanout, types=tag, feat=F,
                                   n_out=n_out, rounds=args.rounds, calls=args.calls, num_dst=blk.num_dst, num_src=blk.num_src, edges=blk.num_edges,
                                   **{"worst_abs_diff_%s_c" % arm: w for arm, w in worst.items()})
                        for arm in worst:   # an arm wins where its slowest round beat the other's fastest
                            rec["c_over_" + arm] = med["c"] / med[arm]
                            rec[arm + "_beats_c_by_more_than_the_spread"] = bool(max(times[arm]) < min(times["c"]))
                            rec["c_beats_%s_by_more_than_the_spread" % arm] = bool(max(times["c"]) < min(times[arm]))
                        # bytes the layer must move, compulsory: every edge's source row, the self rows, both weights once, out
                        esz = 4 if dt == torch.float32 else 2
                        rec["model_bytes"] = (blk.num_edges + blk.num_dst) * F * esz + 2 * F * n_out * esz + blk.num_dst * n_out * esz
                        for arm, t in times.items():
                            rec[arm + "_us"] = med[arm]
                            rec[arm + "_min_max_us"] = [min(t), max(t)]
                        print(json.dumps(rec), flush=True)
        sampler.close()


if __name__ == "__main__":
    main()
