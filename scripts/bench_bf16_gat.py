#!/usr/bin/env python3
"""scripts/bench_bf16_gat.py -- 16-bit features in the fused GAT aggregation (gnnagg_gat_run_typed) against the fp32 path, one JSON
line per config.

  python3 scripts/bench_bf16_gat.py [--configs A1,A8,G] [--steps K] [--warmup W] [--rounds N] [--fp32-only]
  python3 scripts/bench_bf16_gat.py --once CFG [ARM]     a few launches of every arm (or one), for rocprofv3 --kernel-trace / --pmc

Configs: A1 = arxiv-shaped, 1 head x 128 (the fig10a input); A8 = arxiv-shaped, 8 heads x 16; G = reddit-shaped, 8 heads x 32 on an
auto-partitioned handle (fp32: the 2-D blocked order; the 16-bit arms run the chunked plan built beside it).  Arms: fp32 -> fp32,
bf16 -> fp32, bf16 -> bf16, alternated in one process, N rounds (the line takes each arm's median and keeps every round).  Launches run
on one stream made for them, inputs stay on the default stream (bench.time_steps).  Before any timing, every 16-bit arm is checked bit
for bit against the fp32 arm on x.float() (bf16 y: against its round-to-nearest-even).  --fp32-only times the fp32 arm alone and touches
nothing but Aggregator_GAT.run with float32 tensors, so the same file also runs against a checkout that has no typed entry point."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("GNNAGG_BENCH_ROOT", ROOT))   # (another checkout's package and bench.py: the parent-commit arm)
import bench  # noqa: E402
import gnn_computing_amd as gnc  # noqa: E402

bench.np, bench.torch = np, torch   # (bench.py imports them in its main())

ARMS = [("fp32->fp32", torch.float32, torch.float32), ("bf16->fp32", torch.bfloat16, torch.float32),
        ("bf16->bf16", torch.bfloat16, torch.bfloat16)]
CONFIGS = {"A1": ("arxiv", 1, 128), "A8": ("arxiv", 8, 16), "G": ("reddit", 8, 32)}


def gather_model_bytes(V, E, F, H, xsize, ysize):
    """bench.py's config-G model with xsize-byte X and ysize-byte Y elements: per edge one feature row, one id and H fp32 source
    terms; per row one output row and H fp32 centre terms; the row pointers"""
    return E * (xsize * F + 4 + 4 * H) + V * (ysize * F + 4 * H) + 4 * (V + 1)


def setup(cfg, dev):
    name, H, D = CONFIGS[cfg]
    F = H * D
    ptr, idx = gnc.graph.dataset(name, device=dev)
    agg = gnc.Aggregator_GAT(ptr, idx, F, F)
    what = "%s-shaped CSR %dx%d, GAT %d head%s x %d fused, mode=balanced%s" % (
        name, ptr.numel() - 1, idx.numel(), H, "" if H == 1 else "s", D, ", auto-partitioned handle" if cfg == "G" else "")
    return agg, ptr, idx, H, F, what


def make_inputs(V, F, H, dev, dtypes):
    g = torch.Generator(device=dev)
    g.manual_seed(123)
    x32 = torch.randn((V, F), device=dev, generator=g).to(torch.bfloat16).float()   # bf16-representable values in every arm
    att = torch.randn((V, H, 2), device=dev, generator=g)
    return {d: x32.to(d) for d in dtypes}, att


def run_config(cfg, args, dev):
    agg, ptr, idx, H, F, what = setup(cfg, dev)
    V, E = ptr.numel() - 1, idx.numel()
    arms_run = ARMS[:1] if args.fp32_only else ARMS
    xs, att = make_inputs(V, F, H, dev, sorted({xd for _, xd, _ in arms_run}, key=str))
    ys = {yd: torch.empty((V, F), device=dev, dtype=yd) for yd in sorted({yd for _, _, yd in arms_run}, key=str)}
    steps = {name: (lambda xd=xd, yd=yd: agg.run(xs[xd], att, ys[yd], 128, "balanced", heads=H)) for name, xd, yd in arms_run}
    steps["fp32->fp32"]()   # (the first call of each arm also builds its plan and scratch)
    torch.cuda.synchronize()
    parts = agg.balanced_partitions()
    if not args.fp32_only:   # bit-exact checks before any timing
        ref = ys[torch.float32].clone()
        if parts:   # the 16-bit arms run the chunked plan: their fp32 counterpart is a handle that never takes the blocked order
            ref_agg = gnc.Aggregator_GAT(ptr, idx, F, F)
            ref_agg.set_option("partitions", 0)
            ref_agg.run(xs[torch.float32], att, ref, 128, "balanced", heads=H)
            del ref_agg
        steps["bf16->fp32"]()
        ok32 = torch.equal(ys[torch.float32], ref)
        steps["bf16->bf16"]()
        ok16 = torch.equal(ys[torch.bfloat16], ref.to(torch.bfloat16))
        if not (ok32 and ok16):
            raise RuntimeError("%s: 16-bit arm differs from the fp32 arm (bf16->fp32 %s, bf16->bf16 %s)" % (cfg, ok32, ok16))
        del ref
    K, W = (args.steps, args.warmup) if cfg != "G" else (min(args.steps, 20), min(args.warmup, 3))
    samples = {name: [] for name, _, _ in arms_run}
    for _ in range(args.rounds):
        for name, _, _ in arms_run:
            wall, dev_s, _ = bench.time_steps(steps[name], K, W, lambda: None, median=False)
            samples[name].append((wall / K, dev_s))
    arms = {}
    for name, xd, yd in arms_run:
        walls = sorted(s[0] for s in samples[name])
        devs = sorted(s[1] for s in samples[name])
        wall, dev_s = walls[len(walls) // 2], devs[len(devs) // 2]
        B = gather_model_bytes(V, E, F, H, 2 if xd == torch.bfloat16 else 4, 2 if yd == torch.bfloat16 else 4)
        arms[name] = {"ms_per_step": wall * 1e3, "avg_launch_us": dev_s * 1e6, "edges_per_s": E / wall, "gather_model_bytes": B,
                      "gather_model_gbps": B / dev_s / 1e9, "ms_per_step_rounds": [round(s[0] * 1e3, 5) for s in samples[name]],
                      "avg_launch_us_rounds": [round(s[1] * 1e6, 3) for s in samples[name]],
                      "spread_pct": 100.0 * (devs[-1] - devs[0]) / dev_s,
                      "order": ("2-D blocked order (%d source ranges)" % parts if parts and name == "fp32->fp32"
                                else "chunked plan built beside the blocked order" if parts else "chunked plan (k_gat_plan)")}
    for name in arms:
        arms[name]["ratio_to_fp32"] = arms["fp32->fp32"]["avg_launch_us"] / arms[name]["avg_launch_us"]
    return {"config": cfg, "workload": what, "num_v": V, "num_e": E, "feat": F, "heads": H, "steps": K, "warmup": W, "rounds": args.rounds,
            "fp32_only": bool(args.fp32_only), "checked_bit_exact": not args.fp32_only,
            "checked_how": ("bf16->fp32 torch.equal to the fp32 run on x.float(); bf16->bf16 torch.equal to (that run).to(bfloat16); fp32 run "
                            "= the fp32 arm, or on a blocked handle a fp32 handle of the same graph on the chunked plan (partitions = 0)"),
            "source_partitions": parts, "arms": arms,
            "spread_is": "(max - min) / median of avg_launch_us over the rounds, per cent",
            "ratio_is": "fp32->fp32 avg_launch_us / this arm's avg_launch_us (> 1: faster than fp32)"}


def once(cfg, arm, dev):
    agg, ptr, idx, H, F, _ = setup(cfg, dev)
    V = ptr.numel() - 1
    xs, att = make_inputs(V, F, H, dev, [torch.float32, torch.bfloat16])
    ys = {yd: torch.empty((V, F), device=dev, dtype=yd) for yd in (torch.float32, torch.bfloat16)}
    for name, xd, yd in ARMS:
        agg.run(xs[xd], att, ys[yd], 128, "balanced", heads=H)   # plans and scratch outside the traced launches
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        for name, xd, yd in ARMS:
            if arm and name != arm:
                continue
            for _ in range(20 if cfg != "G" else 5):
                agg.run(xs[xd], att, ys[yd], 128, "balanced", heads=H)
            torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="A1,A8,G")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fp32-only", action="store_true", help="time the fp32 arm alone (Aggregator_GAT.run with float32 tensors only)")
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
