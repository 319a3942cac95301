#!/usr/bin/env python3
"""run_v2 and run_dot on the arxiv-shaped graph at EVERY lane geometry the attention launcher can select (the shapes of
tests/geometry_census.py GATV2, fp32 -> fp32 and bf16 -> bf16), without a bias, with a [E, heads] bias and with weights out: the three
instantiations of every geometry.  scripts/bench_gatv2.py and its siblings time two shapes against torch; this one times the library
alone, for comparing two builds of it (GNNAGG_LIB selects the library; run the builds alternately in one session).

A round times `--calls` back-to-back calls between device events on a non-null stream; the figure is the median over `--rounds` rounds,
printed with the minimum and maximum of a round.  One JSON line per (call, shape, types, arm); nothing is asserted.

    python scripts/bench_attn_geometries.py [--rounds 7] [--calls 10] [--dataset arxiv]"""
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--dataset", default="arxiv")
    args = ap.parse_args()
    import torch
    import gnn_computing_amd as gnc
    import geometry_census as gc

    assert torch.cuda.is_available(), "bench_attn_geometries.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    ptrs, idxs = gnc.graph.dataset(args.dataset, device=dev)
    V, E = ptrs.numel() - 1, idxs.numel()
    stream = torch.cuda.Stream()

    def time_round(fn):
        with torch.cuda.stream(stream):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                fn()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / args.calls

    for (H, D) in sorted(gc.GATV2):
        F = H * D
        g = torch.Generator().manual_seed(1)
        x32 = torch.randn((V, F), generator=g)
        a = (torch.randn((H, D), generator=g) / D ** 0.5).to(dev)
        bias = torch.randn((E, H), generator=g).to(dev)
        alpha, stat = torch.empty((E, H), device=dev), torch.empty((V, H, 2), device=dev)
        agg = gnc.Aggregator_GAT(ptrs, idxs, F, F)
        for name, dt in (("fp32->fp32", torch.float32), ("bf16->bf16", torch.bfloat16)):
            x = x32.to(dt).to(dev)
            y = torch.empty((V, F), device=dev, dtype=dt)
            geom = gc.gatv2_geometry(F, H, 2 if dt == torch.bfloat16 else 4)
            for call in ("run_v2", "run_dot"):
                for arm, kw in (("plain", {}), ("bias", dict(bias=bias)), ("weights", dict(weights=alpha, stats=stat))):
                    if call == "run_v2":
                        fn = lambda: agg.run_v2(x, x, a, y, heads=H, **kw)      # noqa: E731
                    else:
                        fn = lambda: agg.run_dot(x, x, x, y, heads=H, **kw)     # noqa: E731
                    with torch.cuda.stream(stream):
                        for _ in range(3):
                            fn()
                    stream.synchronize()
                    t = [time_round(fn) for _ in range(args.rounds)]
                    print(json.dumps(dict(call=call, shape="%d x %d" % (H, D), types=name, arm=arm, segmented=geom[0], group=geom[2], nf=geom[4],
                                          us=statistics.median(t), min_max_us=[min(t), max(t)], rounds=args.rounds, calls=args.calls)), flush=True)
        del agg


if __name__ == "__main__":
    main()
