#!/usr/bin/env python3
"""The multi-aggregation call (Aggregator_GCN.run_multi; gnnagg_gcn_run_multi) against what a caller composed before it, on the
arxiv-shaped graph at F = 128 and F = 64, fp32 -> fp32 and bf16 -> bf16.  Arms:

    multi       (a) run_multi with mean, min, max, std x identity
    multi3      (b) the same x identity, amplification, attenuation
    composed    (c) the composition without the call: run(mean), run(max), run(max) on -x, run(mean) on x * x, the torch elementwise
                ops that make min, var and std of them, and the cat            -- compared with (a)
    composed3       ... with the two scaler multiplies and the wider cat added  -- compared with (b)
    sum         (d) run(reduce="sum") alone: the one-gather floor

and the byte model beside them: E * F * esize + 4 E + 4 (V + 1) in, V * S * A * F * ysize out.  The run() arms take the balanced mode (the
library's fastest order; the only one with 16-bit features).

Arms alternate inside every round on a non-null stream; a round times `--calls` back-to-back calls of one arm between device events; the
figure of an arm is the median over `--rounds` rounds, printed with the minimum and maximum of a round.  The timed (a) output is checked
against the float64 reference of tests/test_multi_aggr_host.py on a fixed row sample plus the longest rows, and against the composition.
One JSON line per (F, types); nothing is asserted about speed.  `--label` names the library in the record; `--only-sum` runs arm (d)
alone, which needs nothing this call added: the script then also runs on a tree and library from before it (the parent comparison).

    python scripts/bench_multi_aggr.py [--rounds 9] [--calls 20] [--dataset arxiv] [--label main] [--only-sum]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--dataset", default="arxiv")
    ap.add_argument("--sample", type=int, default=2048)
    ap.add_argument("--label", default="main")
    ap.add_argument("--only-sum", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_multi_aggr.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    ptrs, idxs = gnc.graph.dataset(args.dataset, device=dev)
    V, E = ptrs.numel() - 1, idxs.numel()
    ptr_np, idx_np = ptrs.cpu().numpy(), idxs.cpu().numpy()
    deg = np.diff(ptr_np)
    sample = np.unique(np.concatenate([np.random.default_rng(7).choice(V, args.sample, replace=False), np.argsort(deg)[-8:]]))
    sub_ptr = np.concatenate([[0], np.cumsum(deg[sample])])
    sub_idx = np.concatenate([idx_np[ptr_np[r]:ptr_np[r + 1]] for r in sample])
    stream = torch.cuda.Stream()
    aggrs, scalers3 = ("mean", "min", "max", "std"), ("identity", "amplification", "attenuation")
    if not args.only_sum:
        from test_multi_aggr_host import BOUNDS, multi_layout, multi_ref, worst_ratio
        delta = gnc.pna_delta(ptr_np)
        degf = torch.from_numpy(deg.astype(np.float32)).to(dev)
        amp = (torch.log(degf + 1.0) / delta)[:, None]
        att = torch.where(degf > 0, delta / torch.log(degf + 1.0), torch.zeros_like(degf))[:, None]

    def time_round(fn):
        with torch.cuda.stream(stream):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                fn()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / args.calls

    for Fw in (128, 64):
        x32 = torch.randn((V, Fw), generator=torch.Generator().manual_seed(1)).to(dev)
        agg = gnc.Aggregator_GCN(ptrs, idxs, None, Fw, Fw)
        for name, dt in (("fp32->fp32", torch.float32), ("bf16->bf16", torch.bfloat16)):
            x = x32.to(dt)
            esz = 2 if dt == torch.bfloat16 else 4
            ysum = torch.empty((V, Fw), device=dev, dtype=dt)
            arms = {"sum": lambda: agg.run(x, ysum, scheduled="balanced", reduce="sum")}
            if not args.only_sum:
                y_a = torch.empty((V, 4 * Fw), device=dev, dtype=dt)
                y_b = torch.empty((V, 12 * Fw), device=dev, dtype=dt)
                t_mean, t_max, t_nmax, t_sq = (torch.empty((V, Fw), device=dev, dtype=dt) for _ in range(4))
                out_c = {}

                def composed(with_scalers):
                    agg.run(x, t_mean, scheduled="balanced", reduce="mean")
                    agg.run(x, t_max, scheduled="balanced", reduce="max")
                    agg.run(-x, t_nmax, scheduled="balanced", reduce="max")
                    agg.run(x * x, t_sq, scheduled="balanced", reduce="mean")
                    std = torch.sqrt(torch.relu(t_sq.float() - t_mean.float() * t_mean.float())).to(dt)
                    out = torch.cat([t_mean, -t_nmax, t_max, std], 1)
                    if with_scalers:
                        out = torch.cat([out, (out * amp).to(dt), (out * att).to(dt)], 1)
                    out_c[with_scalers] = out

                arms.update({"multi": lambda: agg.run_multi(x, y_a, aggrs=aggrs),
                             "multi3": lambda: agg.run_multi(x, y_b, aggrs=aggrs, scalers=scalers3, delta=delta),
                             "composed": lambda: composed(False), "composed3": lambda: composed(True)})
            with torch.cuda.stream(stream):
                for fn in arms.values():       # warm every arm: plans, scratch, the allocator's blocks
                    for _ in range(3):
                        fn()
            stream.synchronize()
            times = {arm: [] for arm in arms}
            for _ in range(args.rounds):
                for arm, fn in arms.items():
                    times[arm].append(time_round(fn))
            med = {arm: statistics.median(t) for arm, t in times.items()}
            spread = {arm: [min(t), max(t)] for arm, t in times.items()}
            in_bytes = E * Fw * esz + 4 * E + 4 * (V + 1)
            rec = dict(input="%s-shaped multi-aggregation F = %d" % (args.dataset, Fw), types=name, library=args.label, V=V, E=E, feat=Fw,
                       rounds=args.rounds, calls=args.calls, sum_us=med["sum"], sum_min_max_us=spread["sum"],
                       model_bytes_sum=in_bytes + V * Fw * esz, model_GBps_sum=(in_bytes + V * Fw * esz) / med["sum"] * 1e-3)
            if not args.only_sum:
                # the timed (a) output: a bf16 y is one rounding of the fp32-y call, which is what the judge sees
                y32 = torch.empty((V, 4 * Fw), device=dev)
                with torch.cuda.stream(stream):
                    agg.run_multi(x, y32, aggrs=aggrs)
                stream.synchronize()
                assert torch.equal(y_a, y32.to(dt)), "the timed output is not the rounding of the fp32-y call"
                ref = multi_ref(sub_ptr, sub_idx, None, x.float().cpu().numpy())
                got = y32.cpu().numpy()[sample]
                worst = 0.0
                for (_, a), cols in multi_layout(aggrs, ("identity",), Fw).items():
                    if a in ("min", "max"):
                        assert np.array_equal(got[:, cols], ref[a]), a
                    else:
                        worst = max(worst, worst_ratio(got[:, cols], ref[a], BOUNDS[a](ref)))
                assert worst <= 1.0, "run_multi outside its bounds on the sampled rows: ratio %.3g" % worst
                assert torch.equal(y_b[:, :4 * Fw], y_a), "the identity blocks depend on the scalers"
                diff_c = float((out_c[False].float() - y_a.float()).abs().max().item())
                bytes_a, bytes_b = in_bytes + V * 4 * Fw * esz, in_bytes + V * 12 * Fw * esz
                rec.update(multi_us=med["multi"], multi3_us=med["multi3"], composed_us=med["composed"], composed3_us=med["composed3"],
                           composed_over_multi=med["composed"] / med["multi"], composed3_over_multi3=med["composed3"] / med["multi3"],
                           multi_over_sum=med["multi"] / med["sum"], multi3_over_sum=med["multi3"] / med["sum"],
                           multi_min_max_us=spread["multi"], multi3_min_max_us=spread["multi3"], composed_min_max_us=spread["composed"],
                           composed3_min_max_us=spread["composed3"],
                           model_bytes_in=in_bytes, model_bytes_multi=bytes_a, model_bytes_multi3=bytes_b,
                           model_multi_over_sum=bytes_a / (in_bytes + V * Fw * esz), model_multi3_over_sum=bytes_b / (in_bytes + V * Fw * esz),
                           model_GBps_multi=bytes_a / med["multi"] * 1e-3, model_GBps_multi3=bytes_b / med["multi3"] * 1e-3,
                           worst_ratio_vs_judge=worst, rows_judged=int(len(sample)), max_abs_diff_vs_composed=diff_c)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
