#!/usr/bin/env python3
"""Pair scoring (gnc.pair_score; gnnagg_pair_score_run) against what a user writes today, on random pairs over a 100 000-row embedding
matrix, fp32 and bf16 -> bf16.  Arms:

    dot   k   the kernel: one launch                                       (gnc.pair_score(hu, hv, u=u, v=v))
          t   the torch expression                                         ((hu[u] * hv[v]).sum(1), int64 ids made outside the timing)
    mlp   f   the fused call: one launch                                   (gnc.pair_score(..., kind="mlp", fused=True))
          c   the composition: two index calls, * or cat, two matmul_NN, biases, ReLUs   (fused=False)

The arms alternate inside every round on a non-null stream; a round times `--calls` back-to-back calls of one arm (wall clock around a
stream synchronisation); the figure of an arm is the median over `--rounds` rounds, with the minimum and maximum of a round.  (f) is
checked against (c) on every shape: fp32 bit for bit, bf16 inside 2^-5 of the largest output; (k) against (t) inside 1e-3 of the largest
|score|.  One JSON line per shape; nothing is asserted about speed.

    python scripts/bench_pair_score.py [--rounds 7] [--calls 10] [--pairs 10000,100000,1000000] [--feats 64,128,256] [--hiddens 64,128,256]
                                       [--n-outs 1,47] [--combines mul,cat] [--label main]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=100000)
    ap.add_argument("--pairs", default="10000,100000,1000000")
    ap.add_argument("--feats", default="64,128,256")
    ap.add_argument("--mlp-feat", type=int, default=128)
    ap.add_argument("--hiddens", default="64,128,256")
    ap.add_argument("--n-outs", default="1,47")
    ap.add_argument("--combines", default="mul,cat")
    ap.add_argument("--kinds", default="dot,mlp")
    ap.add_argument("--label", default="main")
    args = ap.parse_args()
    import torch
    import gnn_computing_amd as gnc

    assert torch.cuda.is_available(), "bench_pair_score.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    ints = lambda s: [int(x) for x in s.split(",")]

    def time_round(fn, calls):
        stream.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            for _ in range(calls):
                fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls

    def measure(arms, rec):
        for fn in arms.values():
            time_round(fn, 2)
        times = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm, fn in arms.items():
                times[arm].append(time_round(fn, args.calls))
        (new, t_new), (old, t_old) = times.items()
        rec.update({"%s_over_%s" % (old, new): statistics.median(t_old) / statistics.median(t_new),
                    "%s_beats_%s_by_more_than_the_spread" % (new, old): bool(max(t_new) < min(t_old)),
                    "%s_beats_%s_by_more_than_the_spread" % (old, new): bool(max(t_old) < min(t_new))})
        for arm, t in times.items():
            rec[arm + "_us"] = statistics.median(t)
            rec[arm + "_min_max_us"] = [min(t), max(t)]
        print(json.dumps(rec), flush=True)

    gen = torch.Generator(device=dev).manual_seed(5)
    for P in ints(args.pairs):
        u = torch.randint(0, args.nodes, (P,), device=dev, generator=gen, dtype=torch.int32)
        v = torch.randint(0, args.nodes, (P,), device=dev, generator=gen, dtype=torch.int32)
        ul, vl = u.long(), v.long()
        for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            base = dict(library=args.label, nodes=args.nodes, pairs=P, types=tag, rounds=args.rounds, calls=args.calls)
            for F in ints(args.feats) if "dot" in args.kinds else ():
                hu, hv = torch.randn((args.nodes, F), device=dev).to(dt), torch.randn((args.nodes, F), device=dev).to(dt)
                out = torch.empty(P, device=dev)
                torch.cuda.synchronize()   # the operands were made on the default stream; the arms run on `stream`
                arms = {"k": lambda: gnc.pair_score(hu, hv, u=u, v=v, out=out), "t": lambda: (hu[ul] * hv[vl]).sum(1)}
                with torch.cuda.stream(stream):
                    got, want = arms["k"]().clone(), (hu[ul].double() * hv[vl].double()).sum(1)
                stream.synchronize()
                worst = float((got.double() - want).abs().max())
                assert worst <= 1e-3 * float(want.abs().max()), (P, tag, F, worst)
                measure(arms, dict(base, kind="dot", feat=F, worst_abs_diff_k_float64=worst))
            F = args.mlp_feat
            hu, hv = torch.randn((args.nodes, F), device=dev).to(dt), torch.randn((args.nodes, F), device=dev).to(dt)
            for combine in args.combines.split(",") if "mlp" in args.kinds else ():
                K = 2 * F if combine == "cat" else F
                for H in ints(args.hiddens):
                    for N in ints(args.n_outs):
                        if not gnc.pair_score_supported("mlp", combine, F, H, N, dt):
                            print(json.dumps(dict(base, kind="mlp", combine=combine, feat=F, hidden=H, n_out=N, supported=False)), flush=True)
                            continue
                        w1, w2 = (torch.randn((K, H), device=dev) / K ** 0.5).to(dt), (torch.randn((H, N), device=dev) / H ** 0.5).to(dt)
                        kw = dict(kind="mlp", combine=combine, w1=w1, w2=w2, b1=torch.randn(H, device=dev), b2=torch.randn(N, device=dev), relu=True)
                        out = torch.empty((P, N), device=dev, dtype=dt)
                        torch.cuda.synchronize()
                        arms = {"f": lambda: gnc.pair_score(hu, hv, u=u, v=v, out=out, fused=True, **kw),
                                "c": lambda: gnc.pair_score(hu, hv, u=u, v=v, fused=False, **kw)}
                        with torch.cuda.stream(stream):
                            got, want = arms["f"]().clone(), arms["c"]()
                        stream.synchronize()
                        if dt == torch.float32:
                            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (P, combine, H, N)
                        worst = float((got.double() - want.double()).abs().max())
                        assert torch.isfinite(got).all().item() and worst <= 2.0 ** -5 * float(want.double().abs().max()), (P, tag, combine, H, N, worst)
                        measure(arms, dict(base, kind="mlp", combine=combine, feat=F, hidden=H, n_out=N, worst_abs_diff_f_c=worst))


if __name__ == "__main__":
    main()
