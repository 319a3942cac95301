#!/usr/bin/env python3
"""scripts/bench_bf16.py -- 16-bit features (gnnagg_gcn_run_typed) against the fp32 path, one JSON line per config.

  python3 scripts/bench_bf16.py [--configs A,P1,R] [--steps K] [--warmup W] [--rounds N]
  python3 scripts/bench_bf16.py --once CFG [ARM]     a few launches of every arm (or one), for rocprofv3 --kernel-trace / --pmc

Configs: A = arxiv-shaped GCN sum F = 128 and P1 = products-shaped GCN sum F = 100, both with the locality reorder applied on load
(bench.load_with_locality_reorder); R = reddit-shaped SAGE mean F = 602 on an auto-partitioned handle (fp32: the 2-D blocked order;
the 16-bit arms run the chunked plan).  Arms: fp32 -> fp32, bf16 -> fp32, bf16 -> bf16, alternated in one process, N rounds (the line
takes each arm's median).  Launches run on one stream made for them, inputs stay on the default stream (bench.time_steps).  Before any
timing, every 16-bit arm is checked bit for bit against the fp32 arm on x.float() (bf16 y: against its round-to-nearest-even)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import gnn_computing_amd as gnc  # noqa: E402

bench.np, bench.torch = np, torch   # (bench.py imports them in its main())

ARMS = [("fp32->fp32", torch.float32, torch.float32), ("bf16->fp32", torch.bfloat16, torch.float32),
        ("bf16->bf16", torch.bfloat16, torch.bfloat16)]


def algorithmic_bytes_typed(V, E, F, xsize, ysize, explicit_val=True):
    """bench.algorithmic_bytes with xsize-byte X and ysize-byte Y elements: E*(xsize*F + 4 [idx] + 4 [val]) + V*ysize*F + 4(V+1)"""
    return E * (xsize * F + 4 + (4 if explicit_val else 0)) + V * ysize * F + (V + 1) * 4


def setup(cfg, dev):
    if cfg in ("A", "P1"):
        name, F = ("arxiv", 128) if cfg == "A" else ("products", 100)
        p, i = gnc.graph.dataset(name, device=dev)
        nptr, nidx, _, _, _ = bench.load_with_locality_reorder(name, p.cpu().numpy(), i.cpu().numpy())
        ptr, idx = torch.from_numpy(nptr).to(dev), torch.from_numpy(nidx).to(dev)
        agg = gnc.Aggregator_GCN(ptr, idx, torch.ones(idx.numel(), device=dev), F, F)
        what = "%s-shaped CSR %dx%d, GCN sum, feat=%d, unit weights, locality reorder applied on load, mode=balanced" % (
            name, ptr.numel() - 1, idx.numel(), F)
        return agg, ptr.numel() - 1, idx.numel(), F, "sum", True, what
    ptr, idx = gnc.graph.dataset("reddit", device=dev)
    agg = gnc.Aggregator_GCN(ptr, idx, None, 602, 602)
    what = "reddit-shaped CSR %dx%d, GraphSAGE mean, feat=602, mode=balanced, auto-partitioned handle" % (ptr.numel() - 1, idx.numel())
    return agg, ptr.numel() - 1, idx.numel(), 602, "mean", False, what


def make_inputs(V, F, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(123)
    xb = torch.randn((V, F), device=dev, generator=g).to(torch.bfloat16)
    return {torch.bfloat16: xb, torch.float32: xb.float()}


def run_config(cfg, args, dev):
    agg, V, E, F, reduce, explicit, what = setup(cfg, dev)
    xs = make_inputs(V, F, dev)
    ys = {yd: torch.empty((V, F), device=dev, dtype=yd) for yd in (torch.float32, torch.bfloat16)}
    steps = {name: (lambda xd=xd, yd=yd: agg.run(xs[xd], ys[yd], 512, "balanced", reduce=reduce)) for name, xd, yd in ARMS}
    # bit-exact checks before any timing (the first call of each arm also builds its plan and scratch)
    steps["fp32->fp32"]()
    torch.cuda.synchronize()
    parts = agg.balanced_partitions()
    ref = ys[torch.float32].clone()
    if parts:   # the 16-bit arms run the chunked plan: their fp32 counterpart is a handle that never takes the blocked order
        ref_agg = gnc.Aggregator_GCN(agg.ptr, agg.idx, agg.val, F, F)
        ref_agg.set_option("partitions", 0)
        ref_agg.run(xs[torch.float32], ref, 512, "balanced", reduce=reduce)
        del ref_agg
    steps["bf16->fp32"]()
    ok32 = torch.equal(ys[torch.float32], ref)
    steps["bf16->bf16"]()
    ok16 = torch.equal(ys[torch.bfloat16], ref.to(torch.bfloat16))
    if not (ok32 and ok16):
        raise RuntimeError("%s: 16-bit arm differs from the fp32 arm (bf16->fp32 %s, bf16->bf16 %s)" % (cfg, ok32, ok16))
    del ref
    K, W = (args.steps, args.warmup) if cfg == "A" else (min(args.steps, 20), min(args.warmup, 3))
    samples = {name: [] for name, _, _ in ARMS}
    for _ in range(args.rounds):
        for name, _, _ in ARMS:
            wall, dev_s, _ = bench.time_steps(steps[name], K, W, lambda: None, median=False)
            samples[name].append((wall / K, dev_s))
    arms = {}
    for name, xd, yd in ARMS:
        walls = sorted(s[0] for s in samples[name])
        devs = sorted(s[1] for s in samples[name])
        wall, dev_s = walls[len(walls) // 2], devs[len(devs) // 2]
        B = algorithmic_bytes_typed(V, E, F, 2 if xd == torch.bfloat16 else 4, 2 if yd == torch.bfloat16 else 4, explicit)
        arms[name] = {"ms_per_step": wall * 1e3, "avg_launch_us": dev_s * 1e6, "edges_per_s": E / wall, "algorithmic_bytes": B,
                      "gather_model_gbps": B / dev_s / 1e9, "ms_per_step_rounds": [round(s[0] * 1e3, 5) for s in samples[name]],
                      "order": ("2-D blocked order (%d source ranges)" % parts if parts and name == "fp32->fp32"
                                else "chunked plan" if parts else "chunked plan (k_gcn_plan)")}
    assert arms["fp32->fp32"]["algorithmic_bytes"] == (bench.algorithmic_bytes(V, E, F, explicit) if explicit else
                                                      E * (4 * F + 4) + V * 4 * F + 4 * (V + 1))
    for name in arms:
        arms[name]["ratio_to_fp32"] = arms["fp32->fp32"]["ms_per_step"] / arms[name]["ms_per_step"]
    return {"config": cfg, "workload": what, "num_v": V, "num_e": E, "feat": F, "steps": K, "warmup": W, "rounds": args.rounds,
            "checked_bit_exact": True,
            "checked_how": ("bf16->fp32 torch.equal to the fp32 run on x.float(); bf16->bf16 torch.equal to (that run).to(bfloat16); fp32 run "
                            "= the fp32 arm, or on a blocked handle a fp32 handle of the same graph on the chunked plan (partitions = 0)"),
            "source_partitions": parts, "arms": arms,
            "ratio_is": "fp32->fp32 ms_per_step / this arm's ms_per_step (> 1: faster than fp32)"}


def once(cfg, arm, dev):
    agg, V, E, F, reduce, _, _ = setup(cfg, dev)
    xs = make_inputs(V, F, dev)
    ys = {yd: torch.empty((V, F), device=dev, dtype=yd) for yd in (torch.float32, torch.bfloat16)}
    for name, xd, yd in ARMS:
        agg.run(xs[xd], ys[yd], 512, "balanced", reduce=reduce)   # plans and scratch outside the traced launches
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        for name, xd, yd in ARMS:
            if arm and name != arm:
                continue
            for _ in range(20 if cfg == "A" else 5):
                agg.run(xs[xd], ys[yd], 512, "balanced", reduce=reduce)
            torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="A,P1,R")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--once", nargs="+", metavar=("CFG", "ARM"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.once:
        once(args.once[0], args.once[1] if len(args.once) > 1 else None, dev)
        return
    for cfg in [c for c in args.configs.split(",") if c]:
        print(json.dumps(run_config(cfg, args, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
