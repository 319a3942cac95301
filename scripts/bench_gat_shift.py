#!/usr/bin/env python3
"""What the max-shifted edge softmax costs (gnnagg_gat_row_shift / gnnagg_gat_run_shifted), on the arxiv-shaped GAT inputs 1 head x 128
(the fig10a input) and 8 heads x 16, fp32 -> fp32 and bf16 -> bf16, balanced mode, a non-null stream, device events around replays of a HIP graph of
20 captured calls (no host time between launches) after a warm-up.  One JSON line per (input, types, call):

    a  gat_run / gat_run_typed            (the unshifted call; the only one a tree without the feature has)
    b  gnnagg_gat_row_shift alone         + its byte model: E ids x 4 B, E gathers of one 8 H-byte piece, V H x 4 B written
    c  gnnagg_gat_run_shifted, shift given
    d  gnnagg_gat_run_shifted, d_shift = NULL (row shift + run)

    python scripts/bench_gat_shift.py [--root TREE] [--tag NAME] [--launches 400] [--warmup 100]

--root: the tree whose gnn_computing_amd is imported (default: this one) -- run it once per tree, alternating, to compare two commits."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="head")
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    import gnn_computing_amd as gnc

    dev = torch.device("cuda", 0)
    ptrs, idxs = gnc.graph.dataset("arxiv", device=dev)
    V, E = ptrs.numel() - 1, idxs.numel()
    stream = torch.cuda.Stream()

    def timed(fn, per_graph=20):
        """us per call: `per_graph` calls captured in one HIP graph (no host time between launches), replayed on the side stream"""
        with torch.cuda.stream(stream):
            fn()                                                   # warm: plans and scratch exist before the capture
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                for _ in range(per_graph):
                    fn()
            for _ in range(max(1, args.warmup // per_graph)):
                graph.replay()
            n = max(1, args.launches // per_graph)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                graph.replay()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / (n * per_graph)

    for H, D in ((1, 128), (8, 16)):
        F = H * D
        g = torch.Generator().manual_seed(1)
        att = (torch.randn((V, H, 2), generator=g) * 0.5).to(dev)
        x32 = torch.randn((V, F), generator=g).to(dev)
        agg = gnc.Aggregator_GAT(ptrs, idxs, F, F)
        has_shift = hasattr(agg, "row_shift")
        for name, dt in (("fp32->fp32", torch.float32), ("bf16->bf16", torch.bfloat16)):
            x, y = x32.to(dt), torch.empty((V, F), device=dev, dtype=dt)
            rec = dict(tag=args.tag, input="arxiv-shaped GAT %d x %d" % (H, D), types=name, V=V, E=E, launches=args.launches)
            rec["a_run_us"] = timed(lambda: agg.run(x, att, y, 128, "balanced", heads=H))
            if has_shift:
                shift = agg.row_shift(att, H)
                rec["b_row_shift_us"] = timed(lambda: agg.row_shift(att, H, out=shift))
                model = E * 4 + E * 8 * H + V * H * 4
                rec["b_model_bytes"] = model
                rec["b_model_GBps"] = model / rec["b_row_shift_us"] * 1e-3
                rec["c_run_shifted_given_us"] = timed(lambda: agg.run(x, att, y, 128, "balanced", heads=H, shift=shift))
                rec["d_run_shifted_null_us"] = timed(lambda: agg.run(x, att, y, 128, "balanced", heads=H, stable=True))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
