#!/usr/bin/env python3
"""scripts/bench_gemm_bf16.py -- the bf16 dense combine (gnnagg_matmul_nn_typed) against the fp32 GEMM, one JSON line per shape.

  python3 scripts/bench_gemm_bf16.py [--shapes MxKxN,...] [--steps K] [--warmup W] [--rounds N]
  python3 scripts/bench_gemm_bf16.py --once MxKxN [ARM]     a few launches of every arm (or one), for rocprofv3 --kernel-trace --stats

Shapes: the five of scripts/bench_gemm.py (the dense stages of the 3-layer model and the reddit / products first layers).  Arms:
fp32 -> fp32 (gnnagg_matmul_nn, untouched by the bf16 work: it is the yardstick), bf16 -> fp32, bf16 -> bf16, and torch.mm on the bf16
operands for context -- alternated in one process on one non-null stream (bench.time_steps), N rounds, each arm's median.  Before any
timing every arm is checked against the float64 product of ITS operands: |C - C64| <= 1e-5 . sum_k |a_k b_k| on a sample of rows (the
bf16 arms' operands are the fp32 arm's, rounded; a bf16 C is checked as one rounding of the bf16 -> fp32 arm's C, bit for bit)."""
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

SHAPES = [(169343, 128, 32), (169343, 128, 64), (169343, 512, 128), (232965, 602, 128), (2449029, 100, 32)]   # (M, K, N): bench_gemm.py
ARMS = ["fp32->fp32", "bf16->fp32", "bf16->bf16", "torch.mm bf16"]
RTOL = 1e-5


def check(name, A, B, C, rows):
    """contract (b) on a sample of rows, in float64 on the host"""
    a64, b64 = A[rows].double().cpu().numpy(), B.double().cpu().numpy()
    err = np.abs(C[rows].double().cpu().numpy() - a64 @ b64)
    ratio = float((err / (np.abs(a64) @ np.abs(b64) + 1e-300)).max())
    if not ratio <= RTOL:
        raise RuntimeError("%s: |C - C64| / sum|a b| = %.3g exceeds %.0e" % (name, ratio, RTOL))
    return ratio


def setup(M, K, N, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(123)
    Ab = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16)
    Bb = (torch.randn((K, N), device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
    A32, B32 = Ab.float(), Bb.float()
    C32, Cb32 = torch.empty((M, N), device=dev), torch.empty((M, N), device=dev)
    Cbb, Ct = torch.empty((M, N), device=dev, dtype=torch.bfloat16), torch.empty((M, N), device=dev, dtype=torch.bfloat16)
    steps = {"fp32->fp32": lambda: gnc.matmul_NN(A32, B32, C32), "bf16->fp32": lambda: gnc.matmul_NN(Ab, Bb, Cb32),
             "bf16->bf16": lambda: gnc.matmul_NN(Ab, Bb, Cbb), "torch.mm bf16": lambda: torch.mm(Ab, Bb, out=Ct)}
    return Ab, Bb, A32, B32, {"fp32->fp32": C32, "bf16->fp32": Cb32, "bf16->bf16": Cbb, "torch.mm bf16": Ct}, steps


def run_shape(M, K, N, args, dev):
    Ab, Bb, A32, B32, outs, steps = setup(M, K, N, dev)
    for name in ARMS:
        steps[name]()
    torch.cuda.synchronize()
    rows = torch.from_numpy(np.unique(np.concatenate([np.arange(min(M, 256)), np.arange(max(M - 256, 0), M),
                                                      np.random.default_rng(1).integers(0, M, 1024)]))).to(dev)
    ratios = {"fp32->fp32": check("fp32->fp32", A32, B32, outs["fp32->fp32"], rows),
              "bf16->fp32": check("bf16->fp32", Ab, Bb, outs["bf16->fp32"], rows)}
    if not torch.equal(outs["bf16->bf16"], outs["bf16->fp32"].to(torch.bfloat16)):
        raise RuntimeError("bf16->bf16 is not one rounding of bf16->fp32")
    samples = {name: [] for name in ARMS}
    for _ in range(args.rounds):
        for name in ARMS:
            _, dev_s, _ = bench.time_steps(steps[name], args.steps, args.warmup, lambda: None, median=False)
            samples[name].append(dev_s * 1e6)
    arms = {}
    for name in ARMS:
        us = sorted(samples[name])[len(samples[name]) // 2]
        ea, ec = (4 if name == "fp32->fp32" else 2), (2 if name in ("bf16->bf16", "torch.mm bf16") else 4)
        byts = ea * (M * K + K * N) + ec * M * N
        arms[name] = {"us": round(us, 2), "gbps": round(byts / us / 1e3, 1), "bytes": byts, "us_rounds": [round(v, 2) for v in samples[name]]}
    f = arms["fp32->fp32"]
    for name in ARMS:
        arms[name]["ratio_to_fp32"] = round(f["us"] / arms[name]["us"], 3)
    return {"M": M, "K": K, "N": N, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "arms": arms,
            "fp32_spread_us": round(max(f["us_rounds"]) - min(f["us_rounds"]), 2),
            "fp32_spread_rel": round((max(f["us_rounds"]) - min(f["us_rounds"])) / f["us"], 4),
            "checked": "every library arm within 1e-5 * sum|a b| of the float64 product of its operands on %d sampled rows; bf16->bf16 "
                       "torch.equal to (bf16->fp32).to(bfloat16)" % rows.numel(),
            "max_err_over_sum_abs": ratios, "us_is": "device time per launch: one event pair around the timed launches / steps",
            "ratio_is": "fp32->fp32 us / this arm's us (> 1: faster than fp32)"}


def once(M, K, N, arm, dev):
    _, _, _, _, _, steps = setup(M, K, N, dev)
    for name in ARMS:
        steps[name]()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        for name in ARMS:
            if arm and name != arm:
                continue
            for _ in range(20):
                steps[name]()
            torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join("%dx%dx%d" % s for s in SHAPES), help="MxKxN,...")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--once", nargs="+", metavar=("MxKxN", "ARM"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.once:
        once(*(int(v) for v in args.once[0].split("x")), args.once[1] if len(args.once) > 1 else None, dev)
        return
    for shape in [s for s in args.shapes.split(",") if s]:
        M, K, N = (int(v) for v in shape.split("x"))
        print(json.dumps(run_shape(M, K, N, args, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
