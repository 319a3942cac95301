#!/usr/bin/env python3
"""The cost of the per-edge score bias of the two attention calls (Aggregator_GAT.run_v2 / run_dot with bias=; gnnagg_gatv2_run_bias,
gnnagg_dot_attn_run_bias) on the arxiv-shaped graph, 1 head x 128 and 8 heads x 16, fp32 -> fp32 and bf16 -> bf16.  Arms per call:

    plain       the call without a bias (the kernels of gnnagg_gatv2_run / gnnagg_dot_attn_run)
    bias_EH     with a [E, heads] bias
    bias_E      with a [E] bias (one value per edge for every head)
    torch       the torch composition of scripts/bench_gatv2.py / bench_dot_attn.py with the bias added to its E x H scores

and the byte model beside them: what one pass of the call moves (bench_gatv2.py / bench_dot_attn.py: ids, gathered rows, the rows read once,
y) and the E * bias_heads * 4 bytes the bias adds to it.

Arms alternate inside every round on a non-null stream; a round times `--calls` back-to-back calls of one arm between device events; the
figure of an arm is the median over `--rounds` rounds, printed with the minimum and maximum of a round.  The biased outputs are checked
against the float64 judges of tests/test_attn_bias_host.py on a fixed row sample plus the longest rows.  One JSON line per (call, shape,
types); nothing is asserted about speed.

    python scripts/bench_attn_bias.py [--rounds 9] [--calls 20] [--dataset arxiv]"""
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
    import torch.nn.functional as F_
    import gnn_computing_amd as gnc
    from test_attn_bias_host import bias_bound, dot_attn_bias_ref, gatv2_bias_ref
    from test_gatv2_host import worst_ratio

    assert torch.cuda.is_available(), "bench_attn_bias.py measures on the GPU only"
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
    stream = torch.cuda.Stream()
    slope = 0.2

    def softmax_sum(e, src, H, D, dt):
        m = torch.full((V, H), float("-inf"), device=dev).scatter_reduce_(0, rows[:, None].expand(E, H), e, "amax")
        w = torch.exp(e - m.index_select(0, rows))
        den = torch.zeros((V, H), device=dev).index_add_(0, rows, w)
        alpha = w / den.index_select(0, rows)
        y = torch.zeros((V, H * D), device=dev).index_add_(0, rows, (src.view(E, H, D).float() * alpha[:, :, None]).view(E, H * D))
        return y.to(dt)

    def torch_dot(q, k, v, H, scale, bias):
        D = q.shape[1] // H
        ks, vs = k.index_select(0, idx64), v.index_select(0, idx64)
        e = (q.index_select(0, rows).view(E, H, D).float() * ks.view(E, H, D).float()).sum(-1) * scale + bias
        return softmax_sum(e, vs, H, D, q.dtype)

    def torch_gatv2(x, a, H, bias):
        D = x.shape[1] // H
        src = x.index_select(0, idx64)
        l = F_.leaky_relu(src + x.index_select(0, rows), slope)
        e = (l.view(E, H, D).float() * a.view(1, H, D)).sum(-1) + bias
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
        bias_eh = (2.0 * torch.randn((E, H), generator=g)).to(dev)
        bias_e = bias_eh[:, 0].contiguous()
        agg = gnc.Aggregator_GAT(ptrs, idxs, Fw, Fw)
        for name, dt in (("fp32->fp32", torch.float32), ("bf16->bf16", torch.bfloat16)):
            qkv = qkv32.to(dt)
            q, k, v = (t.contiguous() for t in (qkv[:, :Fw], qkv[:, Fw:2 * Fw], qkv[:, 2 * Fw:]))
            esz = 2 if dt == torch.bfloat16 else 4
            for call in ("dot", "v2"):
                y = {arm: torch.empty((V, Fw), device=dev, dtype=dt) for arm in ("plain", "bias_EH", "bias_E")}
                y32 = torch.empty((V, Fw), device=dev)
                if call == "dot":
                    run = lambda out, bias: agg.run_dot(q, k, v, out, heads=H, bias=bias)
                    composed = lambda: torch_dot(q, k, v, H, scale, bias_eh)
                    qn, kn, vn = (t.float().cpu().numpy() for t in (q, k, v))
                    judge = lambda b: dot_attn_bias_ref(sub_ptr, sub_idx, qn[sample], kn, vn, H, np.float32(scale), b)
                    model = E * 4 + 2 * E * Fw * esz + 2 * V * Fw * esz + (V + 1) * 4
                else:
                    run = lambda out, bias: agg.run_v2(k, k, a, out, heads=H, slope=slope, bias=bias)
                    composed = lambda: torch_gatv2(k, a, H, bias_eh)
                    kn, an = k.float().cpu().numpy(), a.cpu().numpy()
                    judge = lambda b: gatv2_bias_ref(sub_ptr, sub_idx, kn, kn[sample], an, H, slope, b)
                    model = E * 4 + E * Fw * esz + 2 * V * Fw * esz + (V + 1) * 4
                refs = {}
                for arm, b in (("bias_EH", bias_eh), ("bias_E", bias_e)):
                    ref, L, S = judge(b.cpu().numpy()[sub_edges])
                    refs[arm] = (ref, bias_bound(L, S, H))
                worst = [0.0]

                def check(arm, b):
                    """the timed output (a bf16 y: one rounding of the fp32-y call, which is what the judge sees)"""
                    with torch.cuda.stream(stream):
                        run(y32, b)
                    stream.synchronize()
                    assert torch.equal(y[arm], y32.to(dt)), "the timed output is not the rounding of the fp32-y call"
                    worst[0] = max(worst[0], worst_ratio(y32.cpu().numpy()[sample], *refs[arm]))
                    assert worst[0] <= 1.0, "%s with %s outside the bound on the sampled rows: ratio %.3g" % (call, arm, worst[0])

                arms = {"plain": lambda: run(y["plain"], None), "bias_EH": lambda: run(y["bias_EH"], bias_eh),
                        "bias_E": lambda: run(y["bias_E"], bias_e), "torch": composed}
                with torch.cuda.stream(stream):
                    for fn in arms.values():       # warm every arm: the segment plan, scratch, the allocator's blocks
                        for _ in range(3):
                            fn()
                stream.synchronize()
                times = {arm: [] for arm in arms}
                for _ in range(args.rounds):
                    for arm, fn in arms.items():
                        times[arm].append(time_round(fn))
                        if arm == "bias_EH":
                            check(arm, bias_eh)
                        elif arm == "bias_E":
                            check(arm, bias_e)
                med = {arm: statistics.median(t) for arm, t in times.items()}
                t_ref = composed()
                torch.cuda.synchronize()
                rec = dict(input="%s-shaped %s %d x %d" % (args.dataset, "dot-product attention" if call == "dot" else "GATv2", H, D), call=call,
                           types=name, V=V, E=E, rounds=args.rounds, calls=args.calls,
                           plain_us=med["plain"], bias_EH_us=med["bias_EH"], bias_E_us=med["bias_E"], torch_bias_us=med["torch"],
                           bias_EH_over_plain=med["bias_EH"] / med["plain"], bias_E_over_plain=med["bias_E"] / med["plain"],
                           torch_over_bias_EH=med["torch"] / med["bias_EH"],
                           plain_min_max_us=[min(times["plain"]), max(times["plain"])],
                           bias_EH_min_max_us=[min(times["bias_EH"]), max(times["bias_EH"])],
                           bias_E_min_max_us=[min(times["bias_E"]), max(times["bias_E"])],
                           torch_min_max_us=[min(times["torch"]), max(times["torch"])],
                           model_bytes=model, bias_EH_bytes=E * H * 4, bias_E_bytes=E * 4,
                           model_bias_EH_over_plain=(model + E * H * 4) / model, model_bias_E_over_plain=(model + E * 4) / model,
                           model_GBps_plain=model / med["plain"] * 1e-3, model_GBps_bias_EH=(model + E * H * 4) / med["bias_EH"] * 1e-3,
                           worst_ratio_vs_judge=worst[0], rows_judged=int(len(sample)),
                           max_abs_diff_vs_torch=float((t_ref.float() - y["bias_EH"].float()).abs().max().item()))
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
