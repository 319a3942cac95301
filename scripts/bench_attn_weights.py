#!/usr/bin/env python3
"""The cost of the weights-out form of the two attention calls (Aggregator_GAT.run_v2 / run_dot with weights= and stats=;
gnnagg_gatv2_run_weights, gnnagg_dot_attn_run_weights) on the arxiv-shaped graph, 1 head x 128 and 8 heads x 16, fp32 -> fp32 and
bf16 -> bf16, each without a bias and with a [E, heads] bias.  Arms per (call, shape, types, bias):

    plain       the call without weights (the kernels of gnnagg_*_run / gnnagg_*_run_bias)
    weights     the same call with weights= [E, heads] and stats= [V, heads, 2] (both given: nothing is allocated)
    torch       the torch composition of scripts/bench_attn_bias.py, returning its alpha beside y

and beside them, with --profile, the finishing pass's own device time (k_attn_finish, from a torch.profiler run of the weights call; null
where the profiler gives no kernel times) and the byte model: what one pass of the call moves, and the E * heads * 12 bytes the weights add to it (one 4-byte store
in the walk, one read and one write in the finishing pass; stats are V * heads * 8 bytes more).

Arms alternate inside every round on a non-null stream; a round times `--calls` back-to-back calls of one arm between device events; the
figure of an arm is the median over `--rounds` rounds, printed with the minimum and maximum of a round.  The weights are checked against
the float64 softmax of tests/test_attn_weights_host.py on a fixed row sample plus the longest rows, y against the call without weights
bit for bit.  One JSON line per (call, shape, types, bias); nothing is asserted about speed.

The calls without weights against the parent commit's library are measured with scripts/bench_gatv2.py and scripts/bench_dot_attn.py
as they are, parent / new / parent / new in one session.

    python scripts/bench_attn_weights.py [--rounds 9] [--calls 20] [--dataset arxiv]"""
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
    ap.add_argument("--profile", action="store_true", help="add finish_pass_us: k_attn_finish's device time from a torch.profiler run")
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F_
    import gnn_computing_amd as gnc
    from test_attn_weights_host import softmax_parts

    assert torch.cuda.is_available(), "bench_attn_weights.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    ptrs, idxs = gnc.graph.dataset(args.dataset, device=dev)
    V, E = ptrs.numel() - 1, idxs.numel()
    ptr_np, idx_np = ptrs.cpu().numpy(), idxs.cpu().numpy()
    deg = np.diff(ptr_np)
    sample = np.unique(np.concatenate([np.random.default_rng(7).choice(V, args.sample, replace=False), np.argsort(deg)[-8:]]))
    sub_ptr = np.concatenate([[0], np.cumsum(deg[sample])])
    sub_idx = np.concatenate([idx_np[ptr_np[r]:ptr_np[r + 1]] for r in sample])
    sub_edges = np.concatenate([np.arange(ptr_np[r], ptr_np[r + 1]) for r in sample])
    sub_rows = np.repeat(sample, deg[sample])
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
        return y.to(dt), alpha

    def torch_dot(q, k, v, H, scale, bias):
        D = q.shape[1] // H
        ks, vs = k.index_select(0, idx64), v.index_select(0, idx64)
        e = (q.index_select(0, rows).view(E, H, D).float() * ks.view(E, H, D).float()).sum(-1) * scale
        return softmax_sum(e if bias is None else e + bias, vs, H, D, q.dtype)

    def torch_gatv2(x, a, H, bias):
        D = x.shape[1] // H
        src = x.index_select(0, idx64)
        l = F_.leaky_relu(src + x.index_select(0, rows), slope)
        e = (l.view(E, H, D).float() * a.view(1, H, D)).sum(-1)
        return softmax_sum(e if bias is None else e + bias, src, H, D, x.dtype)

    def time_round(fn):
        with torch.cuda.stream(stream):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                fn()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / args.calls

    def finish_time_us(fn):
        """the device time of k_attn_finish per call, from a profiled run of 10 weights calls; None where the profiler gives no kernel times"""
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                with torch.cuda.stream(stream):
                    for _ in range(10):
                        fn()
                stream.synchronize()
            t = [getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0) for ev in prof.events()
                 if "k_attn_finish" in ev.name]
            t = [x for x in t if x and x > 0]
            return statistics.median(t) if t else None
        except Exception:  # noqa: BLE001
            return None

    for H, D in ((1, 128), (8, 16)):
        Fw = H * D
        scale = 1.0 / math.sqrt(D)
        g = torch.Generator().manual_seed(1)
        qkv32 = torch.randn((V, 3 * Fw), generator=g).to(dev)
        a = (torch.randn((H, D), generator=g) / D ** 0.5).to(dev)
        bias_eh = (2.0 * torch.randn((E, H), generator=g)).to(dev)
        agg = gnc.Aggregator_GAT(ptrs, idxs, Fw, Fw)
        alpha, stat = torch.empty((E, H), device=dev), torch.empty((V, H, 2), device=dev)
        for name, dt in (("fp32->fp32", torch.float32), ("bf16->bf16", torch.bfloat16)):
            qkv = qkv32.to(dt)
            q, k, v = (t.contiguous() for t in (qkv[:, :Fw], qkv[:, Fw:2 * Fw], qkv[:, 2 * Fw:]))
            esz = 2 if dt == torch.bfloat16 else 4
            for call in ("dot", "v2"):
                for bias in (None, bias_eh):
                    y_plain, y_w = (torch.empty((V, Fw), device=dev, dtype=dt) for _ in range(2))
                    if call == "dot":
                        run = lambda out, **kw: agg.run_dot(q, k, v, out, heads=H, bias=bias, **kw)
                        composed = lambda: torch_dot(q, k, v, H, scale, bias)
                        qn, kn = q.float().cpu().numpy().astype(np.float64), k.float().cpu().numpy().astype(np.float64)
                        e64 = float(np.float32(scale)) * (qn[sub_rows] * kn[sub_idx]).reshape(len(sub_idx), H, D).sum(axis=2)
                        model = E * 4 + 2 * E * Fw * esz + 2 * V * Fw * esz + (V + 1) * 4
                    else:
                        run = lambda out, **kw: agg.run_v2(k, k, a, out, heads=H, slope=slope, bias=bias, **kw)
                        composed = lambda: torch_gatv2(k, a, H, bias)
                        kn, an = k.float().cpu().numpy().astype(np.float64), a.cpu().numpy().astype(np.float64)
                        z = kn[sub_rows] + kn[sub_idx]
                        zs = z * float(np.float32(slope))
                        e64 = (an.reshape(1, Fw) * np.where(z > zs, z, zs)).reshape(len(sub_idx), H, D).sum(axis=2)
                        model = E * 4 + E * Fw * esz + 2 * V * Fw * esz + (V + 1) * 4
                    labs = np.abs(e64)
                    if bias is not None:
                        model += E * H * 4
                        b64 = bias.cpu().numpy().astype(np.float64)[sub_edges]
                        e64 = e64 + b64
                        labs = labs + np.abs(b64)
                    a_ref, _, _ = softmax_parts(sub_ptr, e64)
                    # (|e| <= the judges' L term: this bound is the tighter one)
                    starts = sub_ptr[:-1][np.diff(sub_ptr) > 0].astype(np.intp)
                    L = np.zeros((len(sample), H))
                    L[np.diff(sub_ptr) > 0] = np.maximum.reduceat(labs, starts, axis=0)
                    bound = 1e-5 * (1.0 + L[np.repeat(np.arange(len(sample)), np.diff(sub_ptr))]) * a_ref

                    arms = {"plain": lambda: run(y_plain), "weights": lambda: run(y_w, weights=alpha, stats=stat), "torch": composed}
                    with torch.cuda.stream(stream):
                        for fn in arms.values():       # warm every arm: the segment plan, scratch, the allocator's blocks
                            for _ in range(3):
                                fn()
                    stream.synchronize()
                    times = {arm: [] for arm in arms}
                    for _ in range(args.rounds):
                        for arm, fn in arms.items():
                            times[arm].append(time_round(fn))
                    stream.synchronize()
                    assert torch.equal(y_plain, y_w), "y of the weights call differs from the call without weights"
                    err = np.abs(alpha.cpu().numpy().astype(np.float64)[sub_edges] - a_ref)
                    worst = float(np.where(err == 0, 0.0, err / bound).max())
                    assert worst <= 1.0, "%s: alpha outside the bound on the sampled rows: ratio %.3g" % (call, worst)
                    t_y, t_alpha = composed()
                    torch.cuda.synchronize()
                    med = {arm: statistics.median(t) for arm, t in times.items()}
                    fin = finish_time_us(arms["weights"]) if args.profile else None
                    w_bytes, s_bytes = E * H * 12, V * H * 8
                    rec = dict(input="%s-shaped %s %d x %d" % (args.dataset, "dot-product attention" if call == "dot" else "GATv2", H, D),
                               call=call, types=name, bias="[E, heads]" if bias is not None else None, V=V, E=E, rounds=args.rounds,
                               calls=args.calls, plain_us=med["plain"], weights_us=med["weights"], torch_alpha_us=med["torch"],
                               weights_over_plain=med["weights"] / med["plain"], weights_minus_plain_us=med["weights"] - med["plain"],
                               torch_over_weights=med["torch"] / med["weights"], finish_pass_us=fin,
                               plain_min_max_us=[min(times["plain"]), max(times["plain"])],
                               weights_min_max_us=[min(times["weights"]), max(times["weights"])],
                               torch_min_max_us=[min(times["torch"]), max(times["torch"])],
                               model_bytes=model, weights_bytes=w_bytes, stats_bytes=s_bytes,
                               model_weights_over_plain=(model + w_bytes + s_bytes) / model,
                               model_GBps_plain=model / med["plain"] * 1e-3,
                               model_GBps_weights=(model + w_bytes + s_bytes) / med["weights"] * 1e-3,
                               worst_alpha_ratio_vs_float64=worst, rows_judged=int(len(sample)),
                               max_abs_alpha_diff_vs_torch=float((t_alpha - alpha).abs().max().item()),
                               max_abs_y_diff_vs_torch=float((t_y.float() - y_w.float()).abs().max().item()))
                    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
