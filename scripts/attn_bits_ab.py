#!/usr/bin/env python3
"""Bit comparison of the two attention calls between two builds of the library, in ONE process: y, alpha and stat of Aggregator_GAT.run_v2
and run_dot from the library at --a (default: the tree's libgnnagg.so) against the library at --b (an A/B build: scripts/ab_build.sh, or
the parent commit's library copied beside them), selected the way GNNAGG_LIB selects it (gnn_computing_amd/_lib.py: LIB_PATH).

Shapes: every (heads, D) of tests/geometry_census.py GATV2 -- every instantiation of both kernels -- in fp32 and bf16.
Bias:   none, one value per edge with every 5th edge -inf (and one row masked whole), and [E, heads].
Graph:  rows without edges, rows of 1 .. 4 edges, rows on both sides of kGatv2LongEdges (127 / 128 / 129 / 130) and of kGatv2SegEdges
        (511 / 512 / 513), and one row of 1700 edges (four segments, merged by k_gatv2_merge).
Every case runs the call with weights= and stats= (the WEIGHTS arm) and the call without (the BIAS arm, or the plain kernel without a
bias); what is compared is the bytes of y of both and of alpha and stat.  One JSON line per (call, shape, dtype, bias), a last line with
the counts; exit status 1 if any output differs.

    python scripts/attn_bits_ab.py --b gnn_computing_amd/csrc/build/ab/libgnnagg_parent.so"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEGREES = [0, 1, 2, 3, 4, 0, 127, 128, 129, 130, 5, 511, 512, 513, 0, 1700, 7, 64, 65, 33]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", default=os.path.join(ROOT, "gnn_computing_amd", "libgnnagg.so"))
    ap.add_argument("--b", required=True)
    args = ap.parse_args()
    import numpy as np
    import torch
    import gnn_computing_amd as gnc
    from gnn_computing_amd import _lib
    import geometry_census as gc

    assert torch.cuda.is_available(), "attn_bits_ab.py compares on the GPU only"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    deg = np.array(DEGREES * 3, dtype=np.int64)
    V, n_src = len(deg), 257
    ptr_np = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    E = int(ptr_np[-1])
    idx_np = rng.integers(0, n_src, E).astype(np.int32)
    ptr, idx = torch.from_numpy(ptr_np).to(dev), torch.from_numpy(idx_np).to(dev)
    masked_row = DEGREES.index(129)

    def digest(t):
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]

    def run_all(path):
        """{case: {output: digest}} from the library at `path` (a fresh handle per shape, as a fresh process would make it)"""
        _lib.LIB_PATH, _lib._lib = os.path.abspath(path), None
        out = {}
        for (H, D) in sorted(gc.GATV2):
            F = H * D
            g = torch.Generator().manual_seed(H * 1000 + D)
            x32 = torch.randn((max(n_src, V), F), generator=g)
            k32, v32 = torch.randn((n_src, F), generator=g), torch.randn((n_src, F), generator=g)
            a = (torch.randn((H, D), generator=g) / D ** 0.5).to(dev)
            b1 = torch.randn((E,), generator=g)
            b1[::5] = float("-inf")
            b1[int(ptr_np[masked_row]):int(ptr_np[masked_row + 1])] = float("-inf")
            bh = torch.randn((E, H), generator=g)
            agg = gnc.Aggregator_GAT(ptr, idx, F, F)
            for dname, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
                x, k, v = x32.to(dt).to(dev), k32.to(dt).to(dev), v32.to(dt).to(dev)
                for bname, bias in (("none", None), ("edge-inf", b1.to(dev)), ("edge-head", bh.to(dev))):
                    for call in ("run_v2", "run_dot"):
                        y, yw = torch.full((V, F), 7.0, device=dev, dtype=dt), torch.full((V, F), 7.0, device=dev, dtype=dt)
                        alpha, stat = torch.full((E, H), 7.0, device=dev), torch.full((V, H, 2), 7.0, device=dev)
                        if call == "run_v2":
                            agg.run_v2(x, x, a, y, heads=H, bias=bias)
                            agg.run_v2(x, x, a, yw, heads=H, bias=bias, weights=alpha, stats=stat)
                        else:
                            agg.run_dot(x, k, v, y, heads=H, bias=bias)
                            agg.run_dot(x, k, v, yw, heads=H, bias=bias, weights=alpha, stats=stat)
                        torch.cuda.synchronize()
                        out["%s %dx%d %s bias=%s" % (call, H, D, dname, bname)] = dict(y=digest(y), y_weights=digest(yw), alpha=digest(alpha),
                                                                                       stat=digest(stat))
            del agg
        return out

    got_a, got_b = run_all(args.a), run_all(args.b)
    assert got_a.keys() == got_b.keys()
    bad = 0
    for case in got_a:
        differ = [o for o in got_a[case] if got_a[case][o] != got_b[case][o]]
        bad += bool(differ)
        print(json.dumps(dict(case=case, equal=not differ, differ=differ, a=got_a[case], b=got_b[case])), flush=True)
    print(json.dumps(dict(a=os.path.relpath(args.a, ROOT), b=os.path.relpath(args.b, ROOT), V=V, E=E, cases=len(got_a), cases_with_a_difference=bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
