#!/usr/bin/env python3
"""gnc.gat_project on the arxiv-shaped sizes of the 3-layer GAT forward against what it replaces and what it is built on.  Arms, alternated
in rounds of one process on a non-null stream, every arm checked against the others first:
    project      gat_project as shipped (path beside it)
    rowdot       gat_project with GNNAGG_GAT_PROJECT_FUSE=0 (1 forces the epilogue wherever the kernel covers the shape; --rule times both): the GEMM and the row-dot kernel behind it (path 2) -- the other side of the
                 fuse rule wherever `project` took the epilogue; the same launches as `project` elsewhere
    pair         matmul_NN, then matmul_NN(out_dtype=fp32) with the [N, 2] (8 heads: block-diagonal [N, 16]) attention weight: the two dense
                 launches of examples/forward_3layer.py::gat_layer
    gemm         matmul_NN alone: what the attention terms cost on top of it
Per arm the median of the rounds and their min .. max (the run-to-run spread a difference has to exceed).

    python scripts/bench_gat_project.py [--jsonl FILE]     # one JSON line per (shape, dtype)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gnn_computing_amd as gnc  # noqa: E402

dev = torch.device("cuda", 0)
F32, BF16 = torch.float32, torch.bfloat16
SHAPES = [(512, 128, 1), (128, 64, 1), (64, 32, 1), (128, 128, 8)]   # (K, N, heads)
RULE_SHAPES = [(128, 128, 8), (128, 128, 4), (128, 128, 2), (128, 64, 8), (128, 64, 4), (128, 32, 4), (512, 128, 8)]   # D = 16, 32, 64, 8, 16, 8, 16
RULE_ROWS = [1000, 16384, 65536, 169343]


def window(fn, it):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / it


def alternate(arms, rounds, it):
    """{name: [us per call] per round}, the arms taken in turn inside every round; arm = (name, environment value of the switch, fn)"""
    out = {name: [] for name, _, _ in arms}
    for r in range(rounds + 1):   # round 0 warms up
        for name, env, fn in arms:
            os.environ["GNNAGG_GAT_PROJECT_FUSE"] = env
            t = window(fn, it if r else 10)
            if r:
                out[name].append(t)
    os.environ["GNNAGG_GAT_PROJECT_FUSE"] = "1"
    return out


def stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="arxiv")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--jsonl", default=None)
    ap.add_argument("--rule", action="store_true", help="also the fuse rule's table: epilogue against GEMM + row-dot over head layouts and row counts")
    args = ap.parse_args()
    M = gnc.graph.SHAPES[args.dataset][0]
    lines = []
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for K, N, heads in SHAPES:
            D = N // heads
            g = torch.Generator(device=dev).manual_seed(K + N + heads)
            x32 = torch.randn((M, K), device=dev, generator=g)
            w32 = torch.randn((K, N), device=dev, generator=g) / K ** 0.5
            ad32, as32 = (torch.randn((heads, D), device=dev, generator=g) / D ** 0.5 for _ in range(2))
            for dt in (F32, BF16):
                x, w, ad, as_ = (t.to(dt) for t in (x32, w32, ad32, as32))
                wlr = torch.zeros((N, 2 * heads), device=dev, dtype=dt)   # column 2 h: a_dst of head h in its rows, 2 h + 1: a_src
                for h in range(heads):
                    wlr[h * D:(h + 1) * D, 2 * h], wlr[h * D:(h + 1) * D, 2 * h + 1] = ad[h], as_[h]
                feat, att = torch.empty((M, N), device=dev, dtype=dt), torch.empty((M, heads, 2), device=dev)
                feat2, att2 = torch.empty_like(feat), torch.empty((M, 2 * heads), device=dev)
                feat3 = torch.empty_like(feat)

                def project():
                    gnc.gat_project(x, w, ad, as_, heads, feat=feat, att=att)

                def pair():
                    gnc.matmul_NN(x, w, feat2)
                    gnc.matmul_NN(feat2, wlr, att2)

                def gemm():
                    gnc.matmul_NN(x, w, feat3)

                # every arm first: the same feat, and attention terms that agree within the bound of the contract (a scale of sum |feat a|)
                os.environ["GNNAGG_GAT_PROJECT_FUSE"] = "0"
                project()
                att_rowdot, path_rowdot = att.clone(), gnc.last_project_path()
                os.environ["GNNAGG_GAT_PROJECT_FUSE"] = "1"
                att.fill_(float("nan"))
                project()
                path = gnc.last_project_path()
                pair()
                gemm()
                scale = (feat.float().abs() @ wlr.float().abs()).view(M, heads, 2)
                ok = (bool(torch.equal(feat, feat2)) and bool(torch.equal(feat, feat3)) and path_rowdot == 2
                      and bool(((att - att_rowdot).abs() <= 2e-5 * scale).all()) and bool(((att - att2.view(M, heads, 2)).abs() <= 2e-5 * scale).all()))
                t = alternate([("project", "1", project), ("rowdot", "0", project), ("pair", "1", pair), ("gemm", "1", gemm)], args.rounds, args.iters)
                rec = {"dataset": args.dataset, "m": M, "k": K, "n": N, "heads": heads, "dtype": "bf16" if dt == BF16 else "fp32", "path": path,
                       "checked": ok, "rounds": args.rounds, "iters": args.iters, "arms": {name: stats(v) for name, v in t.items()}}
                s = rec["arms"]
                print("%d -> %d heads %d %s: project %.1f us (%.1f .. %.1f, path %d) | gemm + rowdot %.1f (%.1f .. %.1f) | pair %.1f (%.1f .. %.1f) | "
                      "gemm %.1f (%.1f .. %.1f) | checked %s"
                      % (K, N, heads, rec["dtype"], s["project"]["median_us"], s["project"]["min_us"], s["project"]["max_us"], path,
                         s["rowdot"]["median_us"], s["rowdot"]["min_us"], s["rowdot"]["max_us"], s["pair"]["median_us"], s["pair"]["min_us"],
                         s["pair"]["max_us"], s["gemm"]["median_us"], s["gemm"]["min_us"], s["gemm"]["max_us"], ok), flush=True)
                lines.append(json.dumps(rec))
        # the fuse rule's own evidence: epilogue against GEMM + row-dot, bf16 -> bf16, over head layouts and row counts
        for K, N, heads in RULE_SHAPES if args.rule else []:
            for Mr in RULE_ROWS:
                D = N // heads
                g = torch.Generator(device=dev).manual_seed(K + N + heads)
                x = torch.randn((Mr, K), device=dev, generator=g).to(BF16)
                w = (torch.randn((K, N), device=dev, generator=g) / K ** 0.5).to(BF16)
                ad, as_ = ((torch.randn((heads, D), device=dev, generator=g) / D ** 0.5).to(BF16) for _ in range(2))
                feat, att = torch.empty((Mr, N), device=dev, dtype=BF16), torch.empty((Mr, heads, 2), device=dev)

                def project():
                    gnc.gat_project(x, w, ad, as_, heads, feat=feat, att=att)

                paths = []
                for env in ("1", "0"):
                    os.environ["GNNAGG_GAT_PROJECT_FUSE"] = env
                    project()
                    paths.append(gnc.last_project_path())
                t = alternate([("epilogue", "1", project), ("rowdot", "0", project)], args.rounds, args.iters)
                rec = {"rule": True, "m": Mr, "k": K, "n": N, "heads": heads, "dtype": "bf16", "paths": paths, "rounds": args.rounds,
                       "iters": args.iters, "checked": paths == [1, 2], "arms": {name: stats(v) for name, v in t.items()}}
                s = rec["arms"]
                print("rule: M %d, %d -> %d heads %d (D %d) bf16: epilogue %.1f us (%.1f .. %.1f) | gemm + rowdot %.1f (%.1f .. %.1f)"
                      % (Mr, K, N, heads, D, s["epilogue"]["median_us"], s["epilogue"]["min_us"], s["epilogue"]["max_us"], s["rowdot"]["median_us"],
                         s["rowdot"]["min_us"], s["rowdot"]["max_us"]), flush=True)
                lines.append(json.dumps(rec))
    if args.jsonl:
        os.makedirs(os.path.dirname(os.path.abspath(args.jsonl)), exist_ok=True)
        with open(args.jsonl, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not all(json.loads(l)["checked"] for l in lines):
        sys.exit("an arm disagreed with the others")


if __name__ == "__main__":
    main()
