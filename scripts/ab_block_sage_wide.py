#!/usr/bin/env python3
"""Block.sage arms of SEVERAL builds of libgnnagg.so in one process, alternating inside every round (the A/B of the chunked kernel's KC / R
and of the composition on another commit's build).  bench_block_sage.py times one library per process; here every `--libs NAME=PATH` is
loaded beside the shipped library and becomes the library of the package for the length of one call, so all arms see the same block,
operands, stream and session.  Arms: w (fused="wide") and c (fused=False) of the shipped library, w of every further build that has the
kernel, c of one that has not (an earlier commit's build: did the composition move?).  The rest is
bench_block_sage.py's method: the input-layer block of a two-layer batch, mean + self term + bias + ReLU, a round times `--calls` calls of
one arm on a non-null stream, medians of `--rounds` alternating rounds with the minimum and maximum round.  Every w arm is checked against
the shipped library's composition first (fp32 bit for bit, bf16 inside 2^-6 of the largest output).  One JSON line per shape.

    python scripts/ab_block_sage_wide.py --libs kc32r4=gnn_computing_amd/csrc/build/ab/libgnnagg_kc32r4.so --feat 1024 --n-outs 256 --types bf16
    (variant builds: scripts/attic/block_sage_wide_ab.patch and scripts/ab_build.sh)"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="", help="NAME=PATH,... of further builds; `main` is the shipped library")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--datasets", default="arxiv,products")
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--fanouts", default="10,25")
    ap.add_argument("--n-outs", default="128")
    ap.add_argument("--feat", type=int, default=512)
    ap.add_argument("--types", default="fp32,bf16")
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc
    from gnn_computing_amd import _lib

    assert torch.cuda.is_available(), "ab_block_sage_wide.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    F = args.feat

    def load(path):   # a further build: every declared symbol it exports, typed (an older commit's build lacks the newest)
        L = ctypes.CDLL(os.path.abspath(path))
        for name, (res, argtypes) in _lib.SIGNATURES.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype, fn.argtypes = res, argtypes
        L.gnnagg_set_abort_on_error(0)
        return L

    libs = {"main": _lib.lib()}
    for item in filter(None, args.libs.split(",")):
        name, path = item.split("=", 1)
        libs[name] = load(path)

    def under(handle, fn):   # fn with `handle` as the package's library
        def call():
            _lib._lib = handle
            try:
                return fn()
            finally:
                _lib._lib = libs["main"]
        return call

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
        x32 = torch.randn((V, F), device=dev)
        for batch in (int(b) for b in args.batches.split(",")):
            n = min(batch, V)
            seeds = torch.from_numpy(np.random.default_rng(11).choice(V, n, replace=False).astype(np.int32)).to(dev)
            for fanout in (int(f) for f in args.fanouts.split(",")):
                with torch.cuda.stream(stream):
                    blk = sampler.sample_layers(seeds, (fanout, fanout), seed=1)[0]
                stream.synchronize()
                for n_out in (int(v) for v in args.n_outs.split(",")):
                    for tag in args.types.split(","):
                        dt = torch.float32 if tag == "fp32" else torch.bfloat16
                        x = x32 if dt == torch.float32 else x32.to(dt)
                        ws, wn = ((torch.randn((F, n_out), device=dev) / F ** 0.5).to(dt) for _ in range(2))
                        bias = torch.randn(n_out, device=dev)
                        out = torch.empty((blk.num_dst, n_out), device=dev, dtype=dt)
                        torch.cuda.synchronize()

                        def arm_w():
                            return blk.sage(x, wn, ws, bias, reduce="mean", relu=True, out=out, fused="wide")

                        def arm_c():
                            return blk.sage(x, wn, ws, bias, reduce="mean", relu=True, out=out, fused=False)

                        arms = {}
                        for lname, L in libs.items():
                            has_w = hasattr(L, "gnnagg_block_sage_wide_run")
                            if has_w:
                                arms["w:" + lname] = under(L, arm_w)
                            if lname == "main" or not has_w:
                                arms["c:" + lname] = under(L, arm_c)
                        with torch.cuda.stream(stream):
                            want = arms["c:main"]().clone()
                        for arm, fn in arms.items():
                            with torch.cuda.stream(stream):
                                got = fn().clone()
                            stream.synchronize()
                            if dt == torch.float32:
                                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (arm, name, batch, fanout, n_out)
                            worst = float((got.double() - want.double()).abs().max())
                            assert worst <= 2.0 ** -6 * float(want.double().abs().max()), (arm, name, batch, fanout, n_out, tag, worst)
                        for fn in arms.values():
                            time_round(fn, 2)
                        times = {arm: [] for arm in arms}
                        for _ in range(args.rounds):
                            for arm, fn in arms.items():
                                times[arm].append(time_round(fn, args.calls))
                        rec = dict(input="%s-shaped input-layer block" % name, batch=n, fanout=fanout, types=tag, feat=F, n_out=n_out,
                                   rounds=args.rounds, calls=args.calls, num_dst=blk.num_dst, edges=blk.num_edges)
                        # bytes the layer must move, compulsory (bench_block_sage.py), at the shipped w arm's median, beside the ceiling of
                        # gathers of rows (their first KB where they are longer) from a window of the block's source rows, measured here
                        esz = x.element_size()
                        rec["model_bytes"] = (blk.num_edges + blk.num_dst) * F * esz + 2 * F * n_out * esz + blk.num_dst * n_out * esz
                        rec["model_GBps_w"] = round(rec["model_bytes"] / statistics.median(times["w:main"]) / 1e3, 1)
                        with torch.cuda.stream(stream):
                            seg = min(F * esz, 1024)   # (the probe's longest segment: 1 KB of each row)
                            rec["gather_ceiling_GBps"] = round(gnc.probe.row_gather_ceiling(dev, seg, F * esz, blk.num_src * F * esz)["gbps"], 1)
                        for arm, t in times.items():
                            rec[arm] = dict(us=round(statistics.median(t), 1), min=round(min(t), 1), max=round(max(t), 1))
                        print(json.dumps(rec), flush=True)
        sampler.close()


if __name__ == "__main__":
    main()
