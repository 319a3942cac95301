#!/usr/bin/env python3
"""The cost of the per-edge feature rows of the two attention calls (Aggregator_GAT.run_v2 / run_dot with edge=; gnnagg_gatv2_run_edge,
gnnagg_dot_attn_run_edge) on the arxiv-shaped graph, 1 head x 128 and 8 heads x 16, fp32 -> fp32 and bf16 -> bf16.  Arms per call:

    plain       (a) the call without ef (the kernels of gnnagg_gatv2_run / gnnagg_dot_attn_run)
    edge        (b) the edge call
    expanded    (c) what a user did before the edge call: index_select of the source rows to E x F, the add of ef, then the plain call on
                the graph (ptr, arange(E)) whose every edge has its own source row (for GATv2 that call also SUMS xs + ef: the nearest
                thing the plain call can express)
    torch       (d) the torch composition of scripts/bench_gatv2.py / bench_dot_attn.py with the edge term

and the byte model beside them: what one pass of the plain call moves (bench_gatv2.py / bench_dot_attn.py: ids, gathered rows, the rows read
once, y) plus the E * F * esize bytes of ef; the achieved rate against the in-process gather ceiling (gnc.probe.row_gather_ceiling).

Arms alternate inside every round on a non-null stream; a round times `--calls` back-to-back calls of one arm between device events; the
figure of an arm is the median over `--rounds` rounds, printed with the minimum and maximum of a round.  The edge output is checked against
the float64 judges of tests/test_attn_edge_host.py on a fixed row sample plus the longest rows.  One JSON line per (call, shape, types);
nothing is asserted about speed.  `--label` names the library in the record (GNNAGG_LIB selects it: the A/B of the non-temporal ef loads
was two builds run alternately in one session; the switch that built the plain-load arm is in scripts/attic/ab_switches_retired.patch).

    python scripts/bench_attn_edge.py [--rounds 9] [--calls 20] [--dataset arxiv] [--label main]"""
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
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F_
    import gnn_computing_amd as gnc
    from test_attn_edge_host import dot_attn_edge_ref, edge_bound, gatv2_edge_ref
    from test_gatv2_host import worst_ratio

    assert torch.cuda.is_available(), "bench_attn_edge.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    ptrs, idxs = gnc.graph.dataset(args.dataset, device=dev)
    V, E = ptrs.numel() - 1, idxs.numel()
    ptr_np, idx_np = ptrs.cpu().numpy(), idxs.cpu().numpy()
    deg = np.diff(ptr_np)
    sample = np.unique(np.concatenate([np.random.default_rng(7).choice(V, args.sample, replace=False), np.argsort(deg)[-8:]]))
    sub_ptr = np.concatenate([[0], np.cumsum(deg[sample])])
    sub_idx = np.concatenate([idx_np[ptr_np[r]:ptr_np[r + 1]] for r in sample])
    sub_edges = np.concatenate([np.arange(ptr_np[r], ptr_np[r + 1]) for r in sample])
    rows = torch.repeat_interleave(torch.arange(V, device=dev), torch.from_numpy(deg).to(dev))
    idx64 = idxs.long()
    own = torch.arange(E, device=dev, dtype=torch.int32)
    stream = torch.cuda.Stream()
    slope = 0.2

    def softmax_sum(e, src, H, D, dt):
        m = torch.full((V, H), float("-inf"), device=dev).scatter_reduce_(0, rows[:, None].expand(E, H), e, "amax")
        w = torch.exp(e - m.index_select(0, rows))
        den = torch.zeros((V, H), device=dev).index_add_(0, rows, w)
        alpha = w / den.index_select(0, rows)
        y = torch.zeros((V, H * D), device=dev).index_add_(0, rows, (src.view(E, H, D).float() * alpha[:, :, None]).view(E, H * D))
        return y.to(dt)

    def torch_dot(q, k, v, ef, H, scale):
        D = q.shape[1] // H
        ks, vs = k.index_select(0, idx64) + ef, v.index_select(0, idx64) + ef
        e = (q.index_select(0, rows).view(E, H, D).float() * ks.view(E, H, D).float()).sum(-1) * scale
        return softmax_sum(e, vs, H, D, q.dtype)

    def torch_gatv2(x, a, ef, H):
        D = x.shape[1] // H
        src = x.index_select(0, idx64)
        l = F_.leaky_relu(src + ef + x.index_select(0, rows), slope)
        e = (l.view(E, H, D).float() * a.view(1, H, D)).sum(-1)
        return softmax_sum(e, src, H, D, x.dtype)

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
        ef32 = torch.randn((E, Fw), generator=g).to(dev)
        agg = gnc.Aggregator_GAT(ptrs, idxs, Fw, Fw)
        aggx = gnc.Aggregator_GAT(ptrs, own, Fw, Fw)
        for name, dt in (("fp32->fp32", torch.float32), ("bf16->bf16", torch.bfloat16)):
            qkv = qkv32.to(dt)
            q, k, v = (t.contiguous() for t in (qkv[:, :Fw], qkv[:, Fw:2 * Fw], qkv[:, 2 * Fw:]))
            ef = ef32.to(dt)
            esz = 2 if dt == torch.bfloat16 else 4
            efn = ef.float().cpu().numpy()[sub_edges]
            for call in ("dot", "v2"):
                y = {arm: torch.empty((V, Fw), device=dev, dtype=dt) for arm in ("plain", "edge", "expanded")}
                y32 = torch.empty((V, Fw), device=dev)
                if call == "dot":
                    run = lambda out, e: agg.run_dot(q, k, v, out, heads=H, edge=e)
                    expanded = lambda: aggx.run_dot(q, k.index_select(0, idx64) + ef, v.index_select(0, idx64) + ef, y["expanded"], heads=H)
                    composed = lambda: torch_dot(q, k, v, ef, H, scale)
                    qn, kn, vn = (t.float().cpu().numpy() for t in (q, k, v))
                    ref, L, S = dot_attn_edge_ref(sub_ptr, sub_idx, qn[sample], kn, vn, efn, H, np.float32(scale))
                    model = E * 4 + 2 * E * Fw * esz + 2 * V * Fw * esz + (V + 1) * 4
                    # (c): the two gathers read and write E x F each, the two adds read 2 E x F and write E x F each, the call reads 2 E x F
                    expanded_bytes = model + 2 * (2 * E * Fw * esz) + 2 * (3 * E * Fw * esz)
                else:
                    run = lambda out, e: agg.run_v2(k, k, a, out, heads=H, slope=slope, edge=e)
                    expanded = lambda: aggx.run_v2(k.index_select(0, idx64) + ef, k, a, y["expanded"], heads=H, slope=slope)
                    composed = lambda: torch_gatv2(k, a, ef, H)
                    kn, an = k.float().cpu().numpy(), a.cpu().numpy()
                    ref, L, S = gatv2_edge_ref(sub_ptr, sub_idx, kn, kn[sample], an, efn, H, slope)
                    model = E * 4 + E * Fw * esz + 2 * V * Fw * esz + (V + 1) * 4
                    expanded_bytes = model + 2 * E * Fw * esz + 3 * E * Fw * esz
                bound = edge_bound(L, S, H)
                worst = [0.0]

                def check():
                    """the timed output (a bf16 y: one rounding of the fp32-y call, which is what the judge sees)"""
                    with torch.cuda.stream(stream):
                        run(y32, ef)
                    stream.synchronize()
                    assert torch.equal(y["edge"], y32.to(dt)), "the timed output is not the rounding of the fp32-y call"
                    worst[0] = max(worst[0], worst_ratio(y32.cpu().numpy()[sample], ref, bound))
                    assert worst[0] <= 1.0, "%s with edge outside the bound on the sampled rows: ratio %.3g" % (call, worst[0])

                arms = {"plain": lambda: run(y["plain"], None), "edge": lambda: run(y["edge"], ef), "expanded": expanded, "torch": composed}
                with torch.cuda.stream(stream):
                    for fn in arms.values():       # warm every arm: the segment plan, scratch, the allocator's blocks
                        for _ in range(3):
                            fn()
                stream.synchronize()
                times = {arm: [] for arm in arms}
                for _ in range(args.rounds):
                    for arm, fn in arms.items():
                        times[arm].append(time_round(fn))
                        if arm == "edge":
                            check()
                if call == "dot" and dt == torch.float32:
                    assert torch.equal(y["edge"], y["expanded"]), "the edge call differs from the plain call on the expanded graph"
                med = {arm: statistics.median(t) for arm, t in times.items()}
                ceil = gnc.probe.row_gather_ceiling(dev, Fw * esz, Fw * esz, V * Fw * esz)
                t_ref = composed()
                torch.cuda.synchronize()
                ef_bytes = E * Fw * esz
                rec = dict(input="%s-shaped %s %d x %d" % (args.dataset, "dot-product attention" if call == "dot" else "GATv2", H, D), call=call,
                           types=name, library=args.label, V=V, E=E, rounds=args.rounds, calls=args.calls,
                           plain_us=med["plain"], edge_us=med["edge"], expanded_us=med["expanded"], torch_edge_us=med["torch"],
                           edge_over_plain=med["edge"] / med["plain"], expanded_over_edge=med["expanded"] / med["edge"],
                           torch_over_edge=med["torch"] / med["edge"],
                           plain_min_max_us=[min(times["plain"]), max(times["plain"])], edge_min_max_us=[min(times["edge"]), max(times["edge"])],
                           expanded_min_max_us=[min(times["expanded"]), max(times["expanded"])],
                           torch_min_max_us=[min(times["torch"]), max(times["torch"])],
                           model_bytes=model, ef_bytes=ef_bytes, model_edge_over_plain=(model + ef_bytes) / model,
                           expanded_model_bytes=expanded_bytes,
                           model_GBps_plain=model / med["plain"] * 1e-3, model_GBps_edge=(model + ef_bytes) / med["edge"] * 1e-3,
                           gather_ceiling_GBps=ceil["gbps"], edge_fraction_of_ceiling=(model + ef_bytes) / med["edge"] * 1e-3 / ceil["gbps"],
                           worst_ratio_vs_judge=worst[0], rows_judged=int(len(sample)),
                           max_abs_diff_vs_torch=float((t_ref.float() - y["edge"].float()).abs().max().item()))
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
