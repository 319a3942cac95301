#!/usr/bin/env python3
"""run_with_nn_typed on the arxiv-shaped input against the back-to-back pair it replaces: run(relu=) followed by gnc.matmul_NN -- the two
calls a caller had before the typed fused entry point existed.  Arms: fp32, bf16 -> bf16 with a fp32 transformed, bf16 -> bf16 with a
bf16 transformed, each with and without the ReLU.  Pair and fused call are timed in alternating rounds of the same process; per arm the
median of the rounds and their min .. max (the run-to-run spread a difference has to exceed) are printed, with last_nn_path beside them.
Two more arms cover the mixed combinations (bf16 x -> fp32 y with the fp32 product, fp32 x -> bf16 y with the bf16 product).

    python scripts/bench_nn_typed.py [--jsonl FILE]     # one JSON line per shape"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gnn_computing_amd as gnc  # noqa: E402

dev = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16
# name, x dtype, y = weight dtype, transformed dtype; the last two arms: the mixed x / y combinations of the table
ARMS = [("fp32", F32, F32, F32), ("bf16_t_f32", BF16, BF16, F32), ("bf16_t_bf16", BF16, BF16, BF16),
        ("xbf16_yf32", BF16, F32, F32), ("xf32_ybf16", F32, BF16, BF16)]


def window(fn, it):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / it


def alternate(fns, rounds, it):
    """[us per call of every fn] per round, the fns taken in turn inside every round"""
    for fn in fns:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            out[k].append(window(fn, it))
    return out


def stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="arxiv")
    ap.add_argument("--shapes", default="128x32,128x64,64x32,256x64")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--jsonl", default=None)
    args = ap.parse_args()
    V, E = gnc.graph.SHAPES[args.dataset][:2]
    ptr, idx = gnc.graph.powerlaw_csr(V, E, seed=123, device=dev)
    val = torch.randn(E, device=dev)
    lines = []
    for F, OUT in [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]:
        agg = gnc.Aggregator_GCN(ptr, idx, val, F, OUT)
        agg.schedule_balanced(0)
        x32, w32 = torch.randn((V, F), device=dev), torch.randn((F, OUT), device=dev) / F ** 0.5
        rec = {"dataset": args.dataset, "num_v": V, "num_e": E, "feat": F, "feat_out": OUT, "rounds": args.rounds, "iters": args.iters, "arms": {}}
        for name, xdt, wdt, tdt in ARMS:
            x, w = x32.to(xdt), w32.to(wdt)
            y, y2 = torch.empty((V, F), device=dev, dtype=wdt), torch.empty((V, F), device=dev, dtype=wdt)
            t, t2 = torch.empty((V, OUT), device=dev, dtype=tdt), torch.empty((V, OUT), device=dev, dtype=tdt)
            for relu in (False, True):
                def pair():
                    agg.run(x, y2, 128, "balanced", relu=relu)
                    gnc.matmul_NN(y2, w, t2)

                def fused():
                    agg.run_with_nn_typed(x, y, w, t, "balanced", "sum", relu)

                p, f = alternate([pair, fused], args.rounds, args.iters)
                path = agg.last_nn_path()
                same_y = bool(torch.equal(y, y2))
                sp, sf = stats(p), stats(f)
                rec["arms"]["%s%s" % (name, "_relu" if relu else "")] = {"pair": sp, "fused": sf, "last_nn_path": path, "y_equal": same_y}
                print("F=%d OUT=%d %-12s relu %d: pair %.1f us (%.1f .. %.1f) | run_with_nn_typed %.1f us (%.1f .. %.1f) | last_nn_path %d | y equal %s"
                      % (F, OUT, name, relu, sp["median_us"], sp["min_us"], sp["max_us"], sf["median_us"], sf["min_us"], sf["max_us"], path, same_y),
                      flush=True)
        lines.append(json.dumps(rec))
    if args.jsonl:
        os.makedirs(os.path.dirname(os.path.abspath(args.jsonl)), exist_ok=True)
        with open(args.jsonl, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
