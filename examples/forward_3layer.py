#!/usr/bin/env python3
"""3-layer GCN / GAT forward (512 -> 128 -> 64 -> 32) on top of the aggregation library -- the harness of the
reference's Figure7/our.py (layers :171-188, timing loop :247-263: 100 warm-up + 100 timed iterations), written
against the same extension function names (gcn_init / gcn_schedule / gcn_run / gat_init / gat_run ...).

    python examples/forward_3layer.py --model our_GCN --dataset arxiv [--datadir DIR --reorder _thres_0.2]

Without --datadir a synthetic arxiv/reddit/products-shaped CSR is generated (the reference's data sets are an
external download).  The dense layers are the library's own f32-MFMA GEMM by default (--dense torch: torch.mm = rocBLAS /
hipBLASLt, exactly as in the reference script)."""
import argparse
import json
import sys
import os
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gnn_computing_amd as gnc  # noqa: E402


DIMS = [512, 128, 64, 32]                                    # our.py:92-95


class Model:
    """The aggregators, weights and layer functions of Figure7/our.py for one graph (ptrs, idxs: int32 device CSR)."""

    def __init__(self, ptrs, idxs, neighbor_num=32, sched=1, fused_relu=False, dense=torch.mm, seed=123, dtype=torch.float32,
                 stable_softmax=False, fused_nn=False, fused_project=False, heads=1, gatv2=False, transformer=False, edge_bias=False,
                 edge_dim=0):
        dev = ptrs.device
        torch.manual_seed(seed)                               # our.py:76
        self.num_v, self.num_e = ptrs.numel() - 1, idxs.numel()
        self.vals = torch.ones(self.num_e, device=dev)        # our.py:78
        self.at = gnc.gcn_init(ptrs, idxs, self.vals)
        gnc.gcn_schedule(self.at, neighbor_num)               # our.py:84
        self.at_gat = gnc.gat_init(ptrs, idxs)
        gnc.gat_schedule(self.at_gat, neighbor_num)
        self.sched, self.fused_relu, self.dense = sched, fused_relu, dense
        # 1/sqrt(fan_in) scaling keeps activations O(1): the reference's GAT kernel exponentiates raw scores without a
        # max-subtraction (aggr_gat.h:138-143), so un-scaled randn weights overflow exp() in the deeper layers.  stable_softmax
        # (--stable-softmax) runs the GAT layers with the row maximum subtracted (gnnagg_gat_run_shifted), which needs no such scaling
        self.stable_softmax = stable_softmax
        self.weights = [torch.randn(DIMS[k], DIMS[k + 1], device=dev) / DIMS[k] ** 0.5 for k in range(3)]
        self.weights_lr = [torch.randn(DIMS[k + 1], 2, device=dev) / DIMS[k + 1] ** 0.5 for k in range(3)]
        self.h = torch.randn(self.num_v, DIMS[0], device=dev)
        self.outs = [torch.empty(self.num_v, DIMS[k + 1], device=dev) for k in range(3)]
        # dtype = torch.bfloat16: features, weights, intermediates and outputs in bf16 (the same seeded values, cast); accumulation stays
        # fp32 in every kernel (gnnagg_matmul_nn_typed, gnnagg_gcn_run_typed, gnnagg_gat_run_typed); the attention terms stay fp32
        self.dtype = dtype
        if dtype != torch.float32:
            self.weights, self.weights_lr = [w.to(dtype) for w in self.weights], [w.to(dtype) for w in self.weights_lr]
            self.h, self.outs = self.h.to(dtype), [o.to(dtype) for o in self.outs]
        # fused_nn (GCN): layer k's aggregation applies the ReLU and multiplies the finished rows by W_{k+1} in the same call
        # (gnnagg_gcn_run_with_nn_typed): two dense launches fewer, and the activation is not read back for its product
        self.fused_nn = fused_nn
        self.feat2 = [torch.empty(self.num_v, DIMS[k + 1], device=dev, dtype=dtype) for k in range(1, 3)] if fused_nn else None
        # fused_project (GAT): feat2 = feat . W and the attention terms in one call (gnnagg_gat_project) instead of two dense launches, with
        # a_dst = w_lr[:, 0] (the centre term's vector) and a_src = w_lr[:, 1].  heads > 1 (through gat_project only): H heads of
        # DIMS[k + 1] / H columns, attention vectors [H, D] drawn behind every other seeded tensor
        if heads != 1 and not fused_project and not gatv2 and not transformer:
            raise ValueError("heads > 1 runs through gat_project: pass fused_project=True")
        self.fused_project, self.heads = fused_project, heads
        if fused_project:
            if heads == 1:
                self.a_dst = [w[:, 0].contiguous() for w in self.weights_lr]
                self.a_src = [w[:, 1].contiguous() for w in self.weights_lr]
            else:
                vec = lambda k: (torch.randn(heads, DIMS[k + 1] // heads, device=dev) / (DIMS[k + 1] // heads) ** 0.5).to(dtype)
                self.a_dst, self.a_src = [vec(k) for k in range(3)], [vec(k) for k in range(3)]
            self.feat2_gat = [torch.empty(self.num_v, DIMS[k + 1], device=dev, dtype=dtype) for k in range(3)]
            self.att = [torch.empty(self.num_v, heads, 2, device=dev) for k in range(3)]
        # gatv2 (model "our_GATv2"): a layer is feat2 = feat . W and GATv2 attention over feat2 on both sides (Aggregator_GAT.run_v2, the
        # shared-weight form); the attention vectors a_k [heads, D] are fp32 and drawn behind every other seeded tensor
        if gatv2:
            self.a_v2 = [torch.randn(heads, DIMS[k + 1] // heads, device=dev) / (DIMS[k + 1] // heads) ** 0.5 for k in range(3)]
        # transformer (model "our_Transformer"): a layer is ONE projection qkv = feat . [Wq | Wk | Wv] (in x 3 out) and scaled dot-product
        # attention over the edges on its three column views (Aggregator_GAT.run_dot: no copies), scale = 1 / sqrt(D); the packed weights
        # are drawn behind every other seeded tensor
        if transformer:
            self.w_qkv = [(torch.randn(DIMS[k], 3 * DIMS[k + 1], device=dev) / DIMS[k] ** 0.5).to(dtype) for k in range(3)]
        # edge_bias (--edge-bias, the two attention models): a Graphormer-style encoding added to every edge's score, looked up ONCE here:
        # bias[p, h] = table[h, bucket(p)] with a seeded [heads, 8] fp32 table (a generator of its own: every other tensor keeps its
        # values) and bucket(p) = min(7, floor(log2(1 + degree of edge p's source))); [num_e, heads] fp32, the same for the three layers
        self.edge_bias = None
        if edge_bias:
            if not (gatv2 or transformer):
                raise ValueError("edge_bias belongs to the attention models our_GATv2 and our_Transformer")
            self.bias_table = torch.randn(heads, 8, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
            deg = (ptrs[1:] - ptrs[:-1]).to(torch.float64)
            bucket = (torch.frexp(1.0 + deg[idxs.long()])[1] - 1).clamp(max=7).long()   # floor(log2(x)), exact: x = m * 2^e, m in [0.5, 1)
            self.edge_bias = self.bias_table.t()[bucket].contiguous()
        # edge_dim (--edge-dim K, the two attention models): a feature vector per edge.  ONE seeded [num_e, K] attribute tensor and a weight
        # [K, DIMS[k + 1]] per layer (a generator of their own again); layer k's edge rows ef = attr . We[k] enter the score (and, for the
        # transformer, the summed value) through edge= of run_v2 / run_dot -- PyG's GATv2Conv / TransformerConv(edge_dim=K)
        self.edge_dim, self.edge_attr, self.w_edge = int(edge_dim), None, None
        if self.edge_dim:
            if not (gatv2 or transformer):
                raise ValueError("edge_dim belongs to the attention models our_GATv2 and our_Transformer")
            gen = torch.Generator().manual_seed(seed + 2)
            self.edge_attr = torch.randn(self.num_e, self.edge_dim, generator=gen).to(dev).to(dtype)
            self.w_edge = [(torch.randn(self.edge_dim, DIMS[k + 1], generator=gen) / self.edge_dim ** 0.5).to(dev).to(dtype) for k in range(3)]
        self.w_pna = None                                     # model "our_PNA": drawn on its first forward (init_pna)
        self.trace = None                                     # set to a list to record every layer's intermediates

    def gcn_layer(self, feat, out, w):                        # our.py:171-176
        feat2 = self.dense(feat, w)
        if self.fused_relu:
            gnc.gcn_run(self.at, feat2, out, 128, self.sched, relu=True)
            res = out
        else:
            gnc.gcn_run(self.at, feat2, out, 128, self.sched)
            res = F.relu(out)
        if self.trace is not None:
            self.trace.append(dict(feat=feat, w=w, feat2=feat2, out=res.clone()))
        return res

    def forward_gcn_fused_nn(self):
        """feat2_0 = dense(h, W0); layers 0 and 1: out_k = relu(A . feat2_k) and feat2_{k+1} = out_k . W_{k+1} in one call; a plain
        aggregation + ReLU for the last layer"""
        feat, feat2 = self.h, self.dense(self.h, self.weights[0])
        for k in range(3):
            out = self.outs[k]
            if k < 2:
                self.at.run_with_nn_typed(feat2, out, self.weights[k + 1], self.feat2[k], scheduled=self.sched, relu=True)
            else:
                gnc.gcn_run(self.at, feat2, out, 128, self.sched, relu=True)
            if self.trace is not None:
                self.trace.append(dict(feat=feat, w=self.weights[k], feat2=feat2, out=out.clone()))
            if k < 2:
                feat, feat2 = out, self.feat2[k]
        return self.outs[2]

    def dense_f32(self, a, b):
        """a . b with an fp32 result whatever the operands' type (the GAT attention terms)"""
        if self.dtype == torch.float32:
            return self.dense(a, b)
        return self.dense(a, b, out_dtype=torch.float32) if self.dense is gnc.matmul_NN else self.dense(a, b).float()

    def gat_layer(self, feat, out, w, w_lr):                  # our.py:179-188
        feat2 = self.dense(feat, w)
        att_lr = self.dense_f32(feat2, w_lr)
        gnc.gat_run(self.at_gat, feat2, att_lr, out, 128, self.sched, stable=self.stable_softmax)
        if self.trace is not None:
            self.trace.append(dict(feat=feat, w=w, w_lr=w_lr, feat2=feat2, att=att_lr, out=out.clone()))
        return out

    def gat_layer_project(self, feat, out, k):
        """gat_layer with the projection and the attention terms in one call"""
        w = self.weights[k]
        feat2, att = gnc.gat_project(feat, w, self.a_dst[k], self.a_src[k], self.heads, feat=self.feat2_gat[k], att=self.att[k])
        self.at_gat.run(feat2, att, out, 128, self.sched, heads=self.heads, stable=self.stable_softmax)
        if self.trace is not None:
            self.trace.append(dict(feat=feat, w=w, a_dst=self.a_dst[k], a_src=self.a_src[k], heads=self.heads, feat2=feat2.clone(),
                                   att=att.clone(), out=out.clone(), path=gnc.last_project_path()))
        return out

    def edge_rows(self, k):
        """layer k's per-edge feature rows [num_e, DIMS[k + 1]] (None without --edge-dim)"""
        return gnc.matmul_NN(self.edge_attr, self.w_edge[k]) if self.edge_dim else None

    def gatv2_layer(self, feat, out, k):
        feat2 = self.dense(feat, self.weights[k])
        ef = self.edge_rows(k)
        self.at_gat.run_v2(feat2, feat2, self.a_v2[k], out, heads=self.heads, bias=self.edge_bias, edge=ef)
        if self.trace is not None:
            self.trace.append(dict(feat=feat, w=self.weights[k], a=self.a_v2[k], heads=self.heads, feat2=feat2, bias=self.edge_bias, ef=ef,
                                   out=out.clone()))
        return out

    def transformer_layer(self, feat, out, k):
        n = DIMS[k + 1]
        qkv = self.dense(feat, self.w_qkv[k])
        ef = self.edge_rows(k)
        self.at_gat.run_dot(qkv[:, :n], qkv[:, n:2 * n], qkv[:, 2 * n:], out, heads=self.heads, bias=self.edge_bias, edge=ef)
        if self.trace is not None:
            self.trace.append(dict(feat=feat, w=self.w_qkv[k], heads=self.heads, qkv=qkv, bias=self.edge_bias, ef=ef, out=out.clone()))
        return out

    def init_pna(self, seed=126):
        """model "our_PNA": a layer is relu(dense(cat[x, multi(x)], W)) with multi = Aggregator_GCN.run_multi -- mean, min, max and std of the
        neighbourhood from one gather (the aggregation stage of PNAConv, identity scaler).  The weights [5 * in, out] come from a generator
        of their own, on the model's first PNA forward: every other tensor keeps its values, and the constructor its signature"""
        dev, gen = self.h.device, torch.Generator().manual_seed(seed)
        self.w_pna = [(torch.randn(5 * DIMS[k], DIMS[k + 1], generator=gen) / (5 * DIMS[k]) ** 0.5).to(dev).to(self.dtype) for k in range(3)]
        self.multi = [torch.empty(self.num_v, 4 * DIMS[k], device=dev, dtype=self.dtype) for k in range(3)]

    def pna_layer(self, feat, k):
        self.at.run_multi(feat, self.multi[k])
        cat = torch.cat([feat, self.multi[k]], 1)
        res = F.relu(self.dense(cat, self.w_pna[k]))
        if self.trace is not None:
            self.trace.append(dict(feat=feat, w=self.w_pna[k], multi=self.multi[k].clone(), cat=cat, out=res.clone()))
        return res

    def forward(self, model="our_GCN"):
        if self.fused_nn and model == "our_GCN":
            return self.forward_gcn_fused_nn()
        if model == "our_PNA" and self.w_pna is None:
            self.init_pna()
        x = self.h
        for k in range(3):
            if model == "our_GCN":
                x = self.gcn_layer(x, self.outs[k], self.weights[k])
            elif model == "our_GATv2":
                x = self.gatv2_layer(x, self.outs[k], k)
            elif model == "our_Transformer":
                x = self.transformer_layer(x, self.outs[k], k)
            elif model == "our_PNA":
                x = self.pna_layer(x, k)
            elif self.fused_project:
                x = self.gat_layer_project(x, self.outs[k], k)
            else:
                x = self.gat_layer(x, self.outs[k], self.weights[k], self.weights_lr[k])
        return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="our_GCN", choices=["our_GCN", "our_GAT", "our_GATv2", "our_Transformer", "our_PNA"],
                    help="our_PNA: relu(dense(cat[x, mean | min | max | std of the neighbourhood], W)) with the four reductions from one gather "
                         "(Aggregator_GCN.run_multi), honours --dtype and --hip-graph; "
                         "our_GATv2: GATv2 attention (Aggregator_GAT.run_v2) on the projected features; our_Transformer: one [Wq | Wk | Wv] "
                         "projection and scaled dot-product attention on its column views (Aggregator_GAT.run_dot); both honour --dtype, "
                         "--heads, --hip-graph")
    ap.add_argument("--dataset", default="arxiv")
    ap.add_argument("--datadir", default=None)
    ap.add_argument("--reorder", default="")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--neighbor-num", type=int, default=32)   # our.py:84
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--balanced", action="store_true",
                    help="use the library-balanced mode instead of the reference's scheduled=1 on its neighbor-grouping "
                         "schedule (on high-degree graphs that is the source-partitioned order)")
    ap.add_argument("--fused-relu", action="store_true",
                    help="GCN: apply the ReLU inside the aggregation kernel (GNNAGG_FLAG_RELU) instead of F.relu")
    ap.add_argument("--fused-nn", action="store_true",
                    help="GCN: aggregation, ReLU and the NEXT layer's dense combine in one call for layers 0 and 1 "
                         "(gnnagg_gcn_run_with_nn_typed; fp32 and bf16); ignored by the GAT model")
    ap.add_argument("--fused-project", action="store_true",
                    help="GAT: the projection and the attention terms of a layer in one call (gnnagg_gat_project) instead of two dense "
                         "launches; ignored by the GCN model")
    ap.add_argument("--heads", type=int, default=1,
                    help="GAT: attention heads (dividing 128, 64 and 32); more than one runs through gat_project (implies --fused-project)")
    ap.add_argument("--dense", default="library", choices=["library", "torch"],
                    help="dense layers: the library's f32-MFMA GEMM (gnnagg_matmul_nn: bit-exact against the oracle, every stage of "
                         "the forward then is; 512 -> 128: 261 us vs rocBLAS 239 us) or torch.mm as the reference script uses")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"],
                    help="element type of features, weights and layer outputs; bf16: fp32 accumulation everywhere (typed entry points), "
                         "the dense layers on the bf16 MFMA (gnnagg_matmul_nn_typed)")
    ap.add_argument("--stable-softmax", action="store_true",
                    help="GAT: subtract every row's maximal leaky logit before the exp (gnnagg_gat_run_shifted, stable=True): no overflow "
                         "whatever the scale of the weights")
    ap.add_argument("--edge-bias", action="store_true",
                    help="our_GATv2 / our_Transformer: add a per-edge, per-head score bias (run_v2 / run_dot bias=): a seeded [heads, 8] table "
                         "looked up once by min(7, floor(log2(1 + degree of the edge's source)))")
    ap.add_argument("--edge-dim", type=int, default=0,
                    help="our_GATv2 / our_Transformer: a K-element attribute vector per edge (seeded), projected per layer to the layer's width "
                         "and passed as edge= of run_v2 / run_dot (GATv2Conv / TransformerConv(edge_dim=K)); 0: off")
    ap.add_argument("--hip-graph", action="store_true",
                    help="capture one forward in a HIP graph and replay it (the 9-12 launches of a forward are short "
                         "enough on the arxiv-sized graph for launch gaps to show)")
    args = ap.parse_args()
    if args.edge_bias and args.model not in ("our_GATv2", "our_Transformer"):
        ap.error("--edge-bias needs --model our_GATv2 or our_Transformer")
    if args.edge_dim < 0 or (args.edge_dim and args.model not in ("our_GATv2", "our_Transformer")):
        ap.error("--edge-dim needs K >= 0 and --model our_GATv2 or our_Transformer")
    dev = torch.device("cuda", args.gpu)

    if args.datadir:
        ptrs, idxs = gnc.new_load(args.dataset, args.reorder, args.gpu, datadir=args.datadir)
    else:
        ptrs, idxs = gnc.graph.dataset(args.dataset, device=dev)
    m = Model(ptrs, idxs, args.neighbor_num, "balanced" if args.balanced else 1, args.fused_relu,
              gnc.matmul_NN if args.dense == "library" else torch.mm, dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32,
              stable_softmax=args.stable_softmax, fused_nn=args.fused_nn, fused_project=args.fused_project or (args.heads != 1 and args.model not in ("our_GATv2", "our_Transformer")), heads=args.heads,
              gatv2=args.model == "our_GATv2", transformer=args.model == "our_Transformer", edge_bias=args.edge_bias,
              edge_dim=args.edge_dim)
    num_v, num_e = m.num_v, m.num_e

    def forward():
        return m.forward(args.model)

    step, result = forward, None
    if args.hip_graph:
        forward()                                            # plans, scratch and rocBLAS workspaces exist before capture
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            forward()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            result = forward()
        step = graph.replay
    for _ in range(args.iters):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.iters
    y = forward()
    if result is not None:
        assert torch.equal(result, y), "graph replay differs from the eager forward"
    extra = {"edge_bias": True} if args.edge_bias else {}
    if args.edge_dim:
        extra["edge_dim"] = args.edge_dim
    print(json.dumps({**extra, "model": args.model, "dataset": args.dataset, "num_v": num_v, "num_e": num_e,
                      "seconds_per_forward": dt, "hip_graph": bool(args.hip_graph), "fused_relu": bool(args.fused_relu), "fused_nn": bool(args.fused_nn), "fused_project": bool(m.fused_project), "heads": args.heads, "balanced": bool(args.balanced), "dense": args.dense, "dtype": args.dtype, "stable_softmax": bool(args.stable_softmax), "finite": bool(torch.isfinite(y).all().item())}))


if __name__ == "__main__":
    main()
