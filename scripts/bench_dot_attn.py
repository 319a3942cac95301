#!/usr/bin/env python3
"""Scaled dot-product attention over the edges in one call (gnnagg_dot_attn_run, Aggregator_GAT.run_dot) on the arxiv-shaped graph, 1 head x 128
and 8 heads x 16, fp32 -> fp32 and bf16 -> bf16, with q / k / v as the column views of one packed [n, 3F] tensor and as three contiguous
tensors, against

    torch   what a caller does without it, the same layer from torch ops in the same process: index_select of the k and the v rows (an E x F
            tensor each), the per-head product and sum, scatter-amax / exp / index_add softmax, weighted index_add            [the gate]
    v2      the project's GATv2 call at the same shape, Aggregator_GAT.run_v2: the same frame with ONE gathered row per edge     [context]
    model   the bytes one pass moves (E ids, E k rows, E v rows, V q rows, V y rows) over the call's time, beside the in-process gather
            ceiling of gnnagg_probe_row_gather at the same row size                                                          [context]

Arms alternate inside every round on a non-null stream; a round times `--calls` back-to-back calls of one arm between device events; the
figure of an arm is the median over `--rounds` rounds.  Every timed output of run_dot is checked against the float64 judge of
tests/test_dot_attn_host.py on a fixed row sample plus the longest rows.  One JSON line per (shape, types); nothing is asserted about speed.

    python scripts/bench_dot_attn.py [--rounds 9] [--calls 20] [--dataset arxiv]"""
import argparse
import json
import math
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
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc
    from test_dot_attn_host import dot_attn_bound, dot_attn_ref
    from test_gatv2_host import worst_ratio

    assert torch.cuda.is_available(), "bench_dot_attn.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    ptrs, idxs = gnc.graph.dataset(args.dataset, device=dev)
    V, E = ptrs.numel() - 1, idxs.numel()
    ptr_np, idx_np = ptrs.cpu().numpy(), idxs.cpu().numpy()
    deg = np.diff(ptr_np)
    sample = np.unique(np.concatenate([np.random.default_rng(7).choice(V, args.sample, replace=False), np.argsort(deg)[-8:]]))
    sub_ptr = np.concatenate([[0], np.cumsum(deg[sample])])
    sub_idx = np.concatenate([idx_np[ptr_np[r]:ptr_np[r + 1]] for r in sample])
    rows = torch.repeat_interleave(torch.arange(V, device=dev), torch.from_numpy(deg).to(dev))
    idx64 = idxs.long()
    stream = torch.cuda.Stream()

    def torch_dot(q, k, v, H, scale):
        D = q.shape[1] // H
        ks, vs = k.index_select(0, idx64), v.index_select(0, idx64)
        e = (q.index_select(0, rows).view(E, H, D).float() * ks.view(E, H, D).float()).sum(-1) * scale
        m = torch.full((V, H), float("-inf"), device=dev).scatter_reduce_(0, rows[:, None].expand(E, H), e, "amax")
        w = torch.exp(e - m.index_select(0, rows))
        den = torch.zeros((V, H), device=dev).index_add_(0, rows, w)
        alpha = w / den.index_select(0, rows)
        y = torch.zeros((V, H * D), device=dev).index_add_(0, rows, (vs.view(E, H, D).float() * alpha[:, :, None]).view(E, H * D))
        return y.to(q.dtype)

    def time_round(fn):
        with torch.cuda.stream(stream):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                fn()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / args.calls

    for H, D in ((1, 128), (8, 16)):
        Fw = H * D
        scale = 1.0 / math.sqrt(D)
        g = torch.Generator().manual_seed(1)
        qkv32 = torch.randn((V, 3 * Fw), generator=g).to(dev)
        a = (torch.randn((H, D), generator=g) / D ** 0.5).to(dev)
        agg = gnc.Aggregator_GAT(ptrs, idxs, Fw, Fw)
        for name, dt in (("fp32->fp32", torch.float32), ("bf16->bf16", torch.bfloat16)):
            qkv = qkv32.to(dt)
            views = (qkv[:, :Fw], qkv[:, Fw:2 * Fw], qkv[:, 2 * Fw:])
            dense = tuple(t.contiguous() for t in views)
            y = {k: torch.empty((V, Fw), device=dev, dtype=dt) for k in ("packed", "contiguous", "v2")}
            y32 = torch.empty((V, Fw), device=dev)
            x_np = qkv.float().cpu().numpy()
            ref, L, S = dot_attn_ref(sub_ptr, sub_idx, x_np[sample, :Fw], x_np[:, Fw:2 * Fw], x_np[:, 2 * Fw:], H, np.float32(scale))
            bound = dot_attn_bound(L, S, H)
            worst = [0.0]

            def check(ops, out):
                """the timed output (a bf16 y: one rounding of the fp32-y call, which is what the judge sees)"""
                with torch.cuda.stream(stream):
                    agg.run_dot(*ops, y32, heads=H)
                stream.synchronize()
                assert torch.equal(out, y32.to(dt)), "the timed output is not the rounding of the fp32-y call"
                worst[0] = max(worst[0], worst_ratio(y32.cpu().numpy()[sample], ref, bound))
                assert worst[0] <= 1.0, "run_dot outside the bound on the sampled rows: ratio %.3g" % worst[0]

            arms = {"packed": lambda: agg.run_dot(*views, y["packed"], heads=H),
                    "contiguous": lambda: agg.run_dot(*dense, y["contiguous"], heads=H),
                    "torch": lambda: torch_dot(*dense, H, scale),
                    "v2": lambda: agg.run_v2(dense[1], dense[0], a, y["v2"], heads=H)}
            with torch.cuda.stream(stream):
                for fn in arms.values():       # warm every arm: the segment plan, scratch, the allocator's blocks
                    for _ in range(3):
                        fn()
            stream.synchronize()
            times = {k: [] for k in arms}
            for _ in range(args.rounds):
                for k, fn in arms.items():
                    times[k].append(time_round(fn))
                    if k == "packed":
                        check(views, y["packed"])
                    elif k == "contiguous":
                        check(dense, y["contiguous"])
            assert torch.equal(y["packed"], y["contiguous"]), "packed views and contiguous operands differ"
            med = {k: statistics.median(t) for k, t in times.items()}
            esz = 2 if dt == torch.bfloat16 else 4
            model = E * 4 + 2 * E * Fw * esz + 2 * V * Fw * esz + (V + 1) * 4
            ceil = gnc.probe.row_gather_ceiling(dev, Fw * esz, Fw * esz, V * Fw * esz)
            t_ref = torch_dot(*dense, H, scale)
            torch.cuda.synchronize()
            rec = dict(input="%s-shaped dot-product attention %d x %d" % (args.dataset, H, D), types=name, V=V, E=E, rounds=args.rounds,
                       calls=args.calls, run_dot_packed_us=med["packed"], run_dot_contiguous_us=med["contiguous"], torch_us=med["torch"],
                       run_v2_us=med["v2"], torch_over_run_dot_packed=med["torch"] / med["packed"],
                       torch_over_run_dot_contiguous=med["torch"] / med["contiguous"], run_dot_packed_over_run_v2=med["packed"] / med["v2"],
                       run_dot_contiguous_over_run_v2=med["contiguous"] / med["v2"],
                       run_dot_packed_min_max_us=[min(times["packed"]), max(times["packed"])],
                       run_dot_contiguous_min_max_us=[min(times["contiguous"]), max(times["contiguous"])],
                       torch_min_max_us=[min(times["torch"]), max(times["torch"])], run_v2_min_max_us=[min(times["v2"]), max(times["v2"])],
                       model_bytes=model, model_GBps_packed=model / med["packed"] * 1e-3, model_GBps_contiguous=model / med["contiguous"] * 1e-3,
                       gather_ceiling_GBps=ceil["gbps"],
                       worst_ratio_vs_judge=worst[0], rows_judged=int(len(sample)),
                       max_abs_diff_vs_torch=float((t_ref.float() - y["contiguous"].float()).abs().max().item()))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
