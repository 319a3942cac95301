#!/usr/bin/env python3
"""knn_graph (gnnagg_knn_run) against what a user writes today, on batches of synthetic point clouds: 32 x 1 024 points with F = 3, 64,
128 and k = 20; 8 x 4 096 points, F = 64, k = 40; one cloud of 2 048 points, F = 64, k = 20, with the library's splits and with splits = 1;
fp32 and bf16.  Arms:

    f   the fused call: distances on the MFMA and the selection in one kernel (and the merge of the shares where the range is split)
                                                                            (knn_graph(x, k, ptr, fused=True))
    c   the composition: per cloud the norm expansion, a stable sort, the cut  (fused=False)

The arms alternate inside every round on a non-null stream; a round times `--calls` back-to-back calls of one arm (wall clock around a
stream synchronisation); the figure of an arm is the median over `--rounds` rounds, with the minimum and maximum of a round.  Both arms
include what knn_graph does on the host (one read of ptr, the closed form of the result's ptr).  (f) is checked against (c) on every
shape by distance: the k-th distance of every row agrees inside 2^-10 of the row's largest.  One JSON line per shape; nothing is asserted
about speed.

    python scripts/bench_knn.py [--rounds 7] [--calls 10] [--label main]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (clouds, points per cloud, F, k, splits)
SHAPES = [(32, 1024, 3, 20, 0), (32, 1024, 64, 20, 0), (32, 1024, 128, 20, 0), (8, 4096, 64, 40, 0), (1, 2048, 64, 20, 0), (1, 2048, 64, 20, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_knn.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()

    def time_round(fn, calls):
        stream.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            for _ in range(calls):
                fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls

    for clouds, points, F, k, splits in SHAPES:
        n = clouds * points
        ptr = (torch.arange(clouds + 1, dtype=torch.int32) * points).to(dev)
        x32 = torch.randn((n, F), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
        for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            x = x32.to(dt)
            base = dict(input="%d clouds of %d points" % (clouds, points), library=args.label, types=tag, feat=F, k=k, splits=splits,
                        work_bytes=gnc.knn_work_bytes(n, n, F, k, dt, clouds, splits), rounds=args.rounds, calls=args.calls)
            arms = {"f": lambda: gnc.knn_graph(x, k, ptr=ptr, return_dist=True, splits=splits, fused=True),
                    "c": lambda: gnc.knn_graph(x, k, ptr=ptr, return_dist=True, fused=False)}
            torch.cuda.synchronize()   # the operands were made on the default stream; the arms run on `stream`
            with torch.cuda.stream(stream):
                (gb, gd), (wb, wd) = arms["f"](), arms["c"]()
            stream.synchronize()
            assert torch.equal(gb.ptr, wb.ptr) and gb.num_edges == wb.num_edges == n * k
            gd, wd = gd.view(n, k).double(), wd.view(n, k).double()
            worst = float(((gd[:, -1] - wd[:, -1]).abs() / wd[:, -1].clamp_min(1e-30)).max())
            assert worst <= 2.0 ** -10, (clouds, points, F, tag, worst)
            same_ids = float((gb.idx == wb.idx).double().mean())
            for fn in arms.values():
                time_round(fn, 2)
            times = {arm: [] for arm in arms}
            for _ in range(args.rounds):
                for arm, fn in arms.items():
                    times[arm].append(time_round(fn, args.calls))
            rec = dict(base, worst_rel_diff_kth_dist=worst, share_of_equal_ids=same_ids, c_over_f=statistics.median(times["c"]) / statistics.median(times["f"]),
                       f_beats_c_by_more_than_the_spread=bool(max(times["f"]) < min(times["c"])),
                       c_beats_f_by_more_than_the_spread=bool(max(times["c"]) < min(times["f"])))
            for arm, t in times.items():
                rec[arm + "_us"] = statistics.median(t)
                rec[arm + "_min_max_us"] = [min(t), max(t)]
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
