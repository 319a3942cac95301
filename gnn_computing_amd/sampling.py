"""Neighbour sampling (include/gnnagg.h section F): seeds + fanout -> a message-flow block, on the device (csrc/sample.hip) or the
host (csrc/host_graph.cpp).  The sample of a row is a function of (seed, the row's edge positions) alone: the same in every batch, on
either path, bit for bit.  Sampling is not capturable into a HIP graph (sizes are data-dependent and read back once per block).
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .aggregator import (AGGRS, FEATURE_DTYPES, REDUCE, SCALERS, Aggregator_GAT, Aggregator_GCN, _bias_heads, _dev_ptr, _dev_ptr_rows, _edge_rows, _feat_dtype,
                         matmul_NN)
from .scoring import pair_score

_U64 = (1 << 64) - 1


class Block(collections.namedtuple("Block", "ptr idx src_nodes eid num_dst num_src num_edges")):
    """A sampled message-flow block: the rectangular CSR (ptr [num_dst + 1], idx [num_edges]) whose ids index the rows of
    x_src = x[src_nodes] (relabelled; x_dst = x_src[:num_dst]) or of x itself (src_nodes None: global ids, num_src = the graph's rows).
    eid (or None) holds the position of every kept edge in the full CSR: it indexes whatever the caller keeps per edge of the full
    graph -- val, a bias, ef for run_v2 / run_dot."""
    __slots__ = ()

    def gcn(self, val=None):
        """Aggregator_GCN over the block (val: per-edge values of the BLOCK, e.g. full_val[blk.eid])"""
        return Aggregator_GCN(self.ptr, self.idx, val)

    def gat(self):
        return Aggregator_GAT(self.ptr, self.idx)

    def aggregate(self, x, reduce="mean", val=None, val_full=False, gathered=False, out=None, out_dtype=None, relu=False, return_dst=False):
        """The GCN / SAGE aggregation of this block in ONE launch on torch's current stream (gnnagg_block_gcn_run): no handle, no plan, no
        gathered copy of x.  Bit for bit what self.gcn(val).run(x_src, y, 512, 0, reduce) gives.
          x            float32 or bfloat16 [rows, F]; a row-pitched column view is taken as it is.  gathered=False on a relabelled block: the
                       matrix the block was sampled from, read through src_nodes.  gathered=True, or a block of global ids: idx indexes x
                       directly (x[src_nodes], or the previous layer's output).
          val          None (weight 1) or float32: one value per edge of the block, or -- val_full=True -- per edge of the full CSR, read
                       through self.eid
          out          None or a contiguous [num_dst, F] float32 / bfloat16 tensor; out_dtype: the type of the y allocated here (x's by default)
          return_dst   True (or a contiguous [num_dst, F] tensor of x's dtype to fill): also x_dst = x[src_nodes[:num_dst]], copied by the
                       same launch; needs gathered=False on a relabelled block
        Returns y, or (y, x_dst)."""
        return block_gcn_run(self, x, reduce=reduce, val=val, val_full=val_full, gathered=gathered, out=out, out_dtype=out_dtype, relu=relu,
                             return_dst=return_dst)

    def sage(self, x, w_neigh, w_self=None, bias=None, reduce="mean", val=None, val_full=False, gathered=False, out=None, out_dtype=None,
             relu=False, fused=None):
        """A SAGE layer on this block, out = act(x_dst @ w_self + aggregate(x) @ w_neigh + bias), in ONE launch on torch's current stream
        (gnnagg_block_sage_run): the aggregate is never stored, x_dst never copied.  x, reduce, val, val_full, gathered: as in aggregate().
          w_neigh, w_self   contiguous [F, n_out] tensors of x's dtype; w_self None: no self term (a GCN layer, out = aggregate(x) @ w_neigh).
                            The self row of destination i is x[src_nodes[i]], or x[i] (gathered=True, or a block of global ids).
          bias              None or float32 [n_out]
          out               None or a contiguous [num_dst, n_out] tensor: float32 for a float32 x, float32 or bfloat16 for a bfloat16 x;
                            out_dtype: the type of the out allocated here (x's by default)
          fused             True: the kernel, ValueError where gnnagg_block_sage_supported says no (F, n_out <= 256).  "wide": the chunked
                            kernel for rows up to 4096 features (gnnagg_block_sage_wide_run), ValueError where
                            gnnagg_block_sage_wide_supported says no.  False: the composition of existing calls (aggregate, cat,
                            matmul_NN, bias, ReLU) -- for float32 the same bits as either kernel.  None: the kernel where it is
                            supported (sage_prefers_fused), else the chunked kernel where it was measured faster than the
                            composition (sage_prefers_wide), else the composition.
        Returns out."""
        return block_sage_run(self, x, w_neigh, w_self=w_self, bias=bias, reduce=reduce, val=val, val_full=val_full, gathered=gathered, out=out,
                              out_dtype=out_dtype, relu=relu, fused=fused)

    def gin(self, x, w1, w2, b1=None, b2=None, eps=0.0, reduce="sum", val=None, val_full=False, gathered=False, out=None, out_dtype=None,
            relu=False, fused=None):
        """A GIN layer on this block -- GINConv with a two-layer MLP --
        out = act(relu(((1 + eps) * x_dst + aggregate(x)) @ w1 + b1) @ w2 + b2) in ONE launch on torch's current stream
        (gnnagg_block_gin_run): neither the aggregate nor the hidden activations are stored, x_dst is never copied.  x, reduce ("sum",
        "mean" or "max"), val, val_full, gathered, out, out_dtype: as in sage().
          w1, w2       contiguous [F, hidden] and [hidden, n_out] tensors of x's dtype
          b1, b2       None or float32 [hidden] / [n_out]
          eps          the layer's epsilon; the kernel is given float32(1 + eps)
          relu         the activation of out; the hidden ReLU is always applied
          fused        True: the kernel, ValueError where gnnagg_block_gin_supported says no.  False: the composition of existing calls
                       (aggregate, a product and a sum, matmul_NN, bias, ReLU, matmul_NN, bias, ReLU) -- for float32 the same bits.
                       None: the kernel where it is supported and was not measured slower (gin_prefers_fused).
        Returns out."""
        return block_gin_run(self, x, w1, w2, b1=b1, b2=b2, eps=eps, reduce=reduce, val=val, val_full=val_full, gathered=gathered, out=out,
                             out_dtype=out_dtype, relu=relu, fused=fused)

    def edgeconv(self, x, w1, w2, b1=None, b2=None, combine="diff", reduce="max", gathered=False, out=None, out_dtype=None, relu=False, fused=None):
        """An edge-MLP layer on this block -- EdgeConv / DGCNN (combine="diff", reduce="max") or the MPNN / interaction-network message
        (combine="cat") -- out[i] = act(reduce_p (relu(m_p @ w1 + b1) @ w2 + b2)) over the edges p of row i, with
        m_p = cat(x_i, x_s - x_i) ("diff") or cat(x_i, x_s) ("cat"), x_i the destination's own row and x_s the row of idx[p], in ONE
        launch on torch's current stream (gnnagg_block_edgeconv_run): no [E, 2 F] operand and no [E, n_out] message matrix is stored.
        x, gathered, out, out_dtype: as in gin().
          w1, w2       contiguous [2 F, hidden] and [hidden, n_out] tensors of x's dtype
          b1, b2       None or float32 [hidden] / [n_out]
          reduce       "sum", "mean" or "max"; a row without edges is +0 for each
          relu         the activation of out, after the reduction; the hidden ReLU is always applied
          fused        True: the kernel, ValueError where gnnagg_block_edgeconv_supported says no.  False: the composition of existing calls
                       (the index of both row sets, a difference, cat, matmul_NN, bias, ReLU, matmul_NN, bias, then aggregate() over the
                       [E, n_out] messages) -- for float32 the same bits.  None: the kernel where it was measured faster
                       (edgeconv_prefers_fused).
        Returns out."""
        return block_edgeconv_run(self, x, w1, w2, b1=b1, b2=b2, combine=combine, reduce=reduce, gathered=gathered, out=out, out_dtype=out_dtype,
                                  relu=relu, fused=fused)

    def pna(self, x, w, w_self=None, bias=None, aggrs=("mean", "min", "max", "std"), scalers=("identity",), delta=None, val=None, val_full=False,
            gathered=False, out=None, out_dtype=None, relu=False, fused=None):
        """A PNA layer on this block -- PNAConv / MultiAggregation with a linear post-transform and a self term --
        out = act(cat([x_dst, M], 1) @ cat([w_self, w], 0) + bias) in ONE launch on torch's current stream (gnnagg_block_pna_run), with
        M [num_dst, S * A * F] what self.gcn(val).run_multi(x_src, M, aggrs, scalers, delta) gives: M is never stored, x_dst never copied.
        x, val, val_full, gathered, bias, out, out_dtype, relu: as in sage().
          aggrs, scalers   names as in run_multi ("sum", "mean", "min", "max", "var", "std"; "identity", "amplification", "attenuation"),
                           distinct, in any order: the blocks of M (and the row slabs of w) lie scaler-major in the order of the library's bits
          delta            pna_delta(ptr) of the training graph; needed by the two non-identity scalers
          w, w_self        contiguous [S * A * F, n_out] and (or None: no self term) [F, n_out] tensors of x's dtype
          fused            True: the kernel, ValueError where gnnagg_block_pna_supported says no.  False: the composition of existing calls
                           (the gather, gcn(val).run_multi, cat, matmul_NN, bias, ReLU) -- for float32 the same bits on rows of at most
                           128 edges.  None: the kernel where it is supported and was not measured slower (pna_prefers_fused).
        Returns out."""
        return block_pna_run(self, x, w, w_self=w_self, bias=bias, aggrs=aggrs, scalers=scalers, delta=delta, val=val, val_full=val_full,
                             gathered=gathered, out=out, out_dtype=out_dtype, relu=relu, fused=fused)

    def rgcn(self, x, w_rel, etype, w_self=None, bias=None, reduce="mean", etype_full=False, val=None, val_full=False, gathered=False, out=None,
             out_dtype=None, relu=False, fused=None):
        """A relational (typed-edge) GCN layer on this block -- RGCNConv / RelGraphConv without a weight decomposition --
        out = act(x_dst @ w_self + sum_r aggregate_r(x) @ w_rel[r] + bias) in ONE launch on torch's current stream (gnnagg_block_rgcn_run):
        aggregate_r runs over the row's edges of type r only; no sub-block is built, no aggregate stored.  x, val, val_full, gathered, bias,
        out, out_dtype, relu: as in sage().
          w_rel        contiguous [R, F, n_out] of x's dtype; w_self None or contiguous [F, n_out] of x's dtype
          etype        int32, one type per edge of the block, or -- etype_full=True -- per edge of the full CSR, read through self.eid.
                       An edge whose type lies outside [0, R) is skipped: the block with that edge deleted.
          reduce       "sum" or "mean"; the mean is per (row, relation), over the row's edges of that relation
          fused        True: the kernel, ValueError where gnnagg_block_rgcn_supported says no.  False: the composition of existing calls
                       (one filtered sub-block and one aggregate per relation, cat, matmul_NN, bias, ReLU) -- for float32 the same
                       bits.  None: the kernel where it is supported and was not measured slower (rgcn_prefers_fused).
        Returns out."""
        return block_rgcn_run(self, x, w_rel, etype, w_self=w_self, bias=bias, reduce=reduce, etype_full=etype_full, val=val, val_full=val_full,
                              gathered=gathered, out=out, out_dtype=out_dtype, relu=relu, fused=fused)

    def rgcn_basis(self, x, bases, comp, etype, w_self=None, bias=None, reduce="mean", etype_full=False, val=None, val_full=False, gathered=False,
                   out=None, out_dtype=None, relu=False, fused=None):
        """rgcn() with the basis decomposition w_rel[r] = sum_b comp[r, b] * bases[b] -- RGCNConv(num_bases=B), RelGraphConv(regularizer=
        "basis") -- in ONE launch on torch's current stream (gnnagg_block_rgcn_basis_run), for graphs with many relations:
        out = act(x_dst @ w_self + sum_b g_b @ bases[b] + bias), g_b[i] = sum over the row's edges of comp[t, b] * s * x_src with s = val
        (sum) or val / (the row's edges of type t) (mean).  No w_rel is built, and the kernel's LDS holds B + 1 slots per row whatever R is.
        x, etype, etype_full, val, val_full, gathered, w_self, bias, out, out_dtype, relu: as in rgcn().
          bases        contiguous [B, F, n_out] of x's dtype
          comp         contiguous float32 [R, B]
          fused        True: the kernel, ValueError where gnnagg_block_rgcn_basis_supported says no.  False: the route without this call
                       (w_rel = einsum(comp, bases) in x's dtype, then rgcn(..., fused=None)).  None: the kernel where it is supported
                       and was not measured slower -- where rgcn()'s own kernel cannot hold R relations (rgcn_basis_prefers_fused).
        Returns out."""
        return block_rgcn_basis_run(self, x, bases, comp, etype, w_self=w_self, bias=bias, reduce=reduce, etype_full=etype_full, val=val,
                                    val_full=val_full, gathered=gathered, out=out, out_dtype=out_dtype, relu=relu, fused=fused)

    def attend(self, q, k, v=None, kind="dot", a=None, heads=1, scale=None, slope=0.2, bias=None, bias_full=False, edge=None, edge_full=False,
               gathered=False, out=None, out_dtype=None):
        """Edge attention on this block in ONE launch on torch's current stream (gnnagg_block_attn_run): no handle, no plan, no gathered
        copy of any operand.  Rows of at most 128 edges have, bit for bit, what self.gat().run_dot / run_v2 gives on the gathered operands;
        a longer row (fanout = -1 on a hub) is walked by one lane group and holds the float64 bound of those calls instead -- there the
        handle's segmented rows remain the fast path.
          kind="dot"    y[i] = sum_p softmax_p(scale * q[d(i)] . k[s(p)]) v[s(p)] per head; scale=None is 1 / sqrt(F / heads)
          kind="gatv2"  q is xd, k is xs: y[i] = sum_p softmax_p(a[h] . leaky(q[d(i)] + k[s(p)])) k[s(p)]; needs a (float32, heads * D
                        elements) and refuses v
          q, k, v       float32 or bfloat16 [rows, F], one dtype; row-pitched column views (stride(1) == 1) are taken as they are, k and v
                        share stride(0).  gathered=False on a relabelled block: the matrices of the graph the block was sampled from, read
                        through src_nodes (s(p) = src_nodes[idx[p]], d(i) = src_nodes[i]).  gathered=True, or a block of global ids:
                        idx and the row number index them directly.
          bias          None or float32 [E], [E, 1] or [E, heads], added to the score (-inf masks the edge): one row per edge of the block,
                        or -- bias_full=True -- per edge of the full CSR, read through self.eid
          edge          None or [E, F] of q's dtype (stride(1) == 1), added to the scored row (and, for kind="dot", to the summed row):
                        one row per edge of the block, or -- edge_full=True -- per edge of the full CSR, read through self.eid
          out           None or a contiguous [num_dst, F] float32 / bfloat16 tensor; out_dtype: the type of the y allocated here (q's by default)
        Rows without edges are +0.  Returns y."""
        return block_attn_run(self, q, k, v, kind=kind, a=a, heads=heads, scale=scale, slope=slope, bias=bias, bias_full=bias_full, edge=edge,
                              edge_full=edge_full, gathered=gathered, out=out, out_dtype=out_dtype)

    def score(self, hd, hs=None, kind="dot", rel=None, etype=None, combine="mul", w1=None, w2=None, b1=None, b2=None, relu=False, gathered=False,
              out=None, out_dtype=None, fused=None):
        """One score (kind="mlp": one row of n_out values) per EDGE of this block in ONE launch on torch's current stream
        (gnnagg_pair_score_run): pair_score over the block's own CSR -- edge p of destination row i scores (hd row of i, hs row of idx[p]);
        the kernel finds i itself, no row array is built.  hs=None: hs = hd.  gathered=False on a relabelled block: hd and hs are
        matrices of the graph the block was sampled from, read through src_nodes; gathered=True, or a block of global ids: the row
        number and idx index them directly.  etype: one type per edge of the block.  Everything else as in pair_score().
        Returns out, [num_edges] or [num_edges, n_out], in the block's edge order."""
        return pair_score(hd, hd if hs is None else hs, ptr=self.ptr, idx=self.idx, src=None if gathered else self.src_nodes, kind=kind, rel=rel,
                          etype=etype, combine=combine, w1=w1, w2=w2, b1=b1, b2=b2, relu=relu, out=out, out_dtype=out_dtype, fused=fused)


def block_gcn_run(blk, x, reduce="mean", val=None, val_full=False, gathered=False, out=None, out_dtype=None, relu=False, return_dst=False):
    """Block.aggregate as a function (the thin form over gnnagg_block_gcn_run); every dtype and shape refusal is raised before device work"""
    if reduce not in REDUCE:
        raise ValueError("reduce must be one of %s, got %r" % (sorted(REDUCE), reduce))
    mapped = blk.src_nodes is not None and not gathered
    want_dst = return_dst is not False and return_dst is not None
    if val_full and blk.eid is None:
        raise ValueError("val_full=True reads val through blk.eid: sample the block with return_eid=True")
    if val_full and val is None:
        raise ValueError("val_full=True needs val")
    if want_dst and not mapped:
        raise ValueError("return_dst copies x[src_nodes[:num_dst]]: it needs a relabelled block and gathered=False")
    if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
        raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
    # types and shapes
    xdt = _feat_dtype(x, "x")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be 2-D [rows, F] with F >= 1, got %s" % (tuple(x.shape),))
    feat = int(x.shape[1])
    shape = (blk.num_dst, feat)
    if not mapped and int(x.shape[0]) < blk.num_src:
        raise ValueError("x has %d rows, the block's ids index %d (gathered=%s)" % (x.shape[0], blk.num_src, bool(gathered)))
    if val is not None:
        if not isinstance(val, torch.Tensor) or val.dtype != torch.float32:
            raise TypeError("val must be a torch.float32 tensor or None")
        if val.dim() != 1 or (not val_full and int(val.numel()) != blk.num_edges):
            raise ValueError("val must be 1-D%s, got %s" % ("" if val_full else " with one value per edge of the block: [%d]" % blk.num_edges,
                                                             tuple(val.shape)))
    if out is not None:
        _feat_dtype(out, "out")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError("out is %s, out_dtype says %s" % (out.dtype, out_dtype))
        if tuple(out.shape) != shape:
            raise ValueError("out must be [%d, %d], got %s" % (shape + (tuple(out.shape),)))
    x_dst = return_dst if isinstance(return_dst, torch.Tensor) else None
    if x_dst is not None:
        if x_dst.dtype != x.dtype:
            raise TypeError("return_dst must have x's dtype %s, got %s" % (x.dtype, x_dst.dtype))
        if tuple(x_dst.shape) != shape:
            raise ValueError("return_dst must be [%d, %d], got %s" % (shape + (tuple(x_dst.shape),)))
    # device tensors, contiguous where the call wants them dense
    px, pitch = _dev_ptr_rows(x, x.dtype, "x")
    p_ptr, p_idx = _dev_ptr(blk.ptr, torch.int32, "blk.ptr"), _dev_ptr(blk.idx, torch.int32, "blk.idx")
    p_src = _dev_ptr(blk.src_nodes, torch.int32, "blk.src_nodes") if mapped else None
    p_eid = _dev_ptr(blk.eid, torch.int32, "blk.eid") if val_full else None
    p_val = _dev_ptr(val, torch.float32, "val")
    if out is not None:
        _dev_ptr(out, out.dtype, "out")
    if x_dst is not None:
        _dev_ptr(x_dst, x.dtype, "return_dst")
    for name, t in (("blk.ptr", blk.ptr), ("val", val), ("out", out), ("return_dst", x_dst)):
        if t is not None and t.device != x.device:
            raise ValueError("%s lives on %s, x on %s" % (name, t.device, x.device))
    # ---- device work
    if out is None:
        out = torch.empty(shape, dtype=out_dtype or x.dtype, device=x.device)
    ydt = FEATURE_DTYPES[out.dtype]
    if x_dst is None and want_dst:
        x_dst = torch.empty(shape, dtype=x.dtype, device=x.device)
    flags = _lib.FLAG_RELU if relu else 0
    check(lib().gnnagg_block_gcn_run(p_ptr, p_idx if blk.num_edges else None, blk.num_dst, p_src, p_val, p_eid, px, xdt, pitch,
                                     ctypes.c_void_p(out.data_ptr()) if blk.num_dst else None, ydt,
                                     ctypes.c_void_p(x_dst.data_ptr()) if x_dst is not None and blk.num_dst else None, feat, REDUCE[reduce], flags,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return (out, x_dst) if x_dst is not None else out


def block_sage_supported(feat, n_out, dtype):
    """gnnagg_block_sage_supported: does the fused kernel of Block.sage serve [feat] -> [n_out] with operands of `dtype`?"""
    return dtype in FEATURE_DTYPES and bool(lib().gnnagg_block_sage_supported(int(feat), int(n_out), FEATURE_DTYPES[dtype]))


def sage_prefers_fused(num_dst, feat, n_out, dtype):
    """The fused=None rule of Block.sage: the kernel wherever it is supported.  (profiles/block_sage/rule_measurements.txt: the shapes
    measured and what each arm took.)"""
    return block_sage_supported(feat, n_out, dtype)


def block_sage_wide_supported(feat, n_out, dtype):
    """gnnagg_block_sage_wide_supported: does the chunked kernel of Block.sage (fused="wide") serve [feat] -> [n_out] with operands of `dtype`?"""
    return dtype in FEATURE_DTYPES and bool(lib().gnnagg_block_sage_wide_supported(int(feat), int(n_out), FEATURE_DTYPES[dtype]))


def sage_prefers_wide(num_dst, feat, n_out, dtype):
    """The fused=None rule of Block.sage past the range of the narrow kernel: the chunked kernel only for shape classes where its slowest
    round beat the composition's fastest round (profiles/block_sage_wide/rule_measurements.txt: every shape measured and what each arm
    took).  That is one class: float32, feat a multiple of 4 in 260 .. 512, n_out in 64 .. 128 and at most 21 250 destination rows --
    260 / 384 / 512 -> 128 and 512 -> 64 were measured on four blocks each and won on all sixteen (1.11 - 2.51 x); widths and n_out
    between measured points are taken with them, nothing outside them.  21 250 rows is the largest measured block that won at all four
    shapes; the next larger one measured (34 682 rows) lost at 512 -> 128, and nothing between the two was timed.  Larger float32
    blocks, 602 -> 128 and 1024 -> 256 won on some shapes and lost on others, and bfloat16 lost or tied on every shape: those take the
    composition.  Block.sage adds what only it knows: every measured x had 16-byte lanes (a pitch that is a multiple of 4 floats, a
    16-byte aligned first row); an x without them takes the composition."""
    return (dtype == torch.float32 and 260 <= feat <= 512 and feat % 4 == 0 and 64 <= n_out <= 128 and num_dst <= 21250
            and block_sage_wide_supported(feat, n_out, dtype))


def block_sage_run(blk, x, w_neigh, w_self=None, bias=None, reduce="mean", val=None, val_full=False, gathered=False, out=None, out_dtype=None,
                   relu=False, fused=None):
    """Block.sage as a function (the thin form over gnnagg_block_sage_run); every dtype and shape refusal is raised before device work"""
    if reduce not in REDUCE:
        raise ValueError("reduce must be one of %s, got %r" % (sorted(REDUCE), reduce))
    mapped = blk.src_nodes is not None and not gathered
    if val_full and blk.eid is None:
        raise ValueError("val_full=True reads val through blk.eid: sample the block with return_eid=True")
    if val_full and val is None:
        raise ValueError("val_full=True needs val")
    if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
        raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
    # types and shapes
    xdt = _feat_dtype(x, "x")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be 2-D [rows, F] with F >= 1, got %s" % (tuple(x.shape),))
    feat = int(x.shape[1])
    need_rows = blk.num_src if not mapped else 0
    if w_self is not None and not mapped:
        need_rows = max(need_rows, blk.num_dst)
    if int(x.shape[0]) < need_rows:
        raise ValueError("x has %d rows, the block's ids index %d (gathered=%s)" % (x.shape[0], need_rows, bool(gathered)))
    if val is not None:
        if not isinstance(val, torch.Tensor) or val.dtype != torch.float32:
            raise TypeError("val must be a torch.float32 tensor or None")
        if val.dim() != 1 or (not val_full and int(val.numel()) != blk.num_edges):
            raise ValueError("val must be 1-D%s, got %s" % ("" if val_full else " with one value per edge of the block: [%d]" % blk.num_edges,
                                                             tuple(val.shape)))
    for name, w in (("w_neigh", w_neigh), ("w_self", w_self)):
        if w is None and name == "w_self":
            continue
        if not isinstance(w, torch.Tensor) or w.dtype != x.dtype:
            raise TypeError("%s must be a tensor of x's dtype %s, got %s" % (name, x.dtype, getattr(w, "dtype", type(w).__name__)))
        if w.dim() != 2 or int(w.shape[0]) != feat or int(w.shape[1]) < 1 or w.shape != w_neigh.shape:
            raise ValueError("%s must be [%d, n_out] with n_out >= 1%s, got %s" % (name, feat, "" if w is w_neigh else ", as w_neigh", tuple(w.shape)))
    n_out = int(w_neigh.shape[1])
    shape = (blk.num_dst, n_out)
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
            raise TypeError("bias must be a torch.float32 tensor or None")
        if tuple(bias.shape) != (n_out,):
            raise ValueError("bias must be [%d], got %s" % (n_out, tuple(bias.shape)))
    if out is not None:
        _feat_dtype(out, "out")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError("out is %s, out_dtype says %s" % (out.dtype, out_dtype))
        if tuple(out.shape) != shape:
            raise ValueError("out must be [%d, %d], got %s" % (shape + (tuple(out.shape),)))
    odt = out.dtype if out is not None else (out_dtype or x.dtype)
    if x.dtype == torch.float32 and odt != torch.float32:
        raise TypeError("out_dtype: float32 operands give a float32 out, got %s" % (odt,))
    wide = isinstance(fused, str) and fused == "wide"
    if fused is not None and not wide:
        fused = bool(fused)   # (1, 0 and numpy's bools mean True and False, as they always have)
    if fused is True and not block_sage_supported(feat, n_out, x.dtype):
        raise ValueError("fused=True: gnnagg_block_sage_supported(feat=%d, n_out=%d, %s) says no" % (feat, n_out, x.dtype))
    if wide and not block_sage_wide_supported(feat, n_out, x.dtype):
        raise ValueError("fused=\"wide\": gnnagg_block_sage_wide_supported(feat=%d, n_out=%d, %s) says no" % (feat, n_out, x.dtype))
    # device tensors, contiguous where the call wants them dense
    px, pitch = _dev_ptr_rows(x, x.dtype, "x")
    p_ptr, p_idx = _dev_ptr(blk.ptr, torch.int32, "blk.ptr"), _dev_ptr(blk.idx, torch.int32, "blk.idx")
    p_src = _dev_ptr(blk.src_nodes, torch.int32, "blk.src_nodes") if mapped else None
    p_eid = _dev_ptr(blk.eid, torch.int32, "blk.eid") if val_full else None
    p_val = _dev_ptr(val, torch.float32, "val")
    p_wn, p_ws, p_b = _dev_ptr(w_neigh, x.dtype, "w_neigh"), _dev_ptr(w_self, x.dtype, "w_self"), _dev_ptr(bias, torch.float32, "bias")
    if out is not None:
        _dev_ptr(out, out.dtype, "out")
    for name, t in (("blk.ptr", blk.ptr), ("val", val), ("w_neigh", w_neigh), ("w_self", w_self), ("bias", bias), ("out", out)):
        if t is not None and t.device != x.device:
            raise ValueError("%s lives on %s, x on %s" % (name, t.device, x.device))
    # ---- device work
    if fused is None:   # the narrow kernel wherever it serves, else the chunked one where it was measured faster, else the composition
        lanes16 = pitch % 4 == 0 and x.data_ptr() % 16 == 0   # (the lanes sage_prefers_wide was measured with)
        fused = sage_prefers_fused(blk.num_dst, feat, n_out, x.dtype) or (lanes16 and sage_prefers_wide(blk.num_dst, feat, n_out, x.dtype) and "wide")
    if not fused:   # the composition a caller writes with the existing calls
        y = block_gcn_run(blk, x, reduce=reduce, val=val, val_full=val_full, gathered=gathered, return_dst=mapped and w_self is not None)
        if w_self is not None:
            y, x_dst = y if mapped else (y, x[:blk.num_dst])
            res = matmul_NN(torch.cat([x_dst, y], 1), torch.cat([w_self, w_neigh], 0), out_dtype=torch.float32)
        else:
            res = matmul_NN(y, w_neigh, out_dtype=torch.float32)
        if bias is not None:
            res = res + bias
        if relu:
            res = res.clamp_min(0)
        if out is None:
            return res.to(odt)
        out.copy_(res)
        return out
    if out is None:
        out = torch.empty(shape, dtype=odt, device=x.device)
    run = lib().gnnagg_block_sage_wide_run if fused == "wide" else lib().gnnagg_block_sage_run
    check(run(p_ptr, p_idx if blk.num_edges else None, blk.num_dst, p_src, p_val, p_eid, px, xdt, pitch, feat, p_ws, p_wn,
              p_b, n_out, ctypes.c_void_p(out.data_ptr()) if blk.num_dst else None, FEATURE_DTYPES[out.dtype],
              REDUCE[reduce], _lib.FLAG_RELU if relu else 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def block_gin_supported(feat, hidden, n_out, dtype):
    """gnnagg_block_gin_supported: does the fused kernel of Block.gin serve [feat] -> [hidden] -> [n_out] with operands of `dtype`?"""
    return dtype in FEATURE_DTYPES and bool(lib().gnnagg_block_gin_supported(int(feat), int(hidden), int(n_out), FEATURE_DTYPES[dtype]))


def gin_prefers_fused(num_dst, feat, hidden, n_out, dtype):
    """The fused=None rule of Block.gin: the kernel wherever it is supported.  (profiles/block_gin/rule_measurements.txt: the shapes
    measured and what each arm took.)"""
    return block_gin_supported(feat, hidden, n_out, dtype)


def block_gin_run(blk, x, w1, w2, b1=None, b2=None, eps=0.0, reduce="sum", val=None, val_full=False, gathered=False, out=None, out_dtype=None,
                  relu=False, fused=None):
    """Block.gin as a function (the thin form over gnnagg_block_gin_run); every dtype and shape refusal is raised before device work"""
    if reduce not in REDUCE:
        raise ValueError("reduce must be one of %s, got %r" % (sorted(REDUCE), reduce))
    mapped = blk.src_nodes is not None and not gathered
    if val_full and blk.eid is None:
        raise ValueError("val_full=True reads val through blk.eid: sample the block with return_eid=True")
    if val_full and val is None:
        raise ValueError("val_full=True needs val")
    if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
        raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
    with np.errstate(over="ignore"):
        self_scale = float(np.float32(1.0 + eps))
    if not math.isfinite(self_scale):
        raise ValueError("eps = %r: 1 + eps must be a finite float32" % (eps,))
    # types and shapes
    xdt = _feat_dtype(x, "x")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be 2-D [rows, F] with F >= 1, got %s" % (tuple(x.shape),))
    feat = int(x.shape[1])
    need_rows = max(blk.num_src, blk.num_dst) if not mapped else 0
    if int(x.shape[0]) < need_rows:
        raise ValueError("x has %d rows, the block's ids index %d (gathered=%s)" % (x.shape[0], need_rows, bool(gathered)))
    if val is not None:
        if not isinstance(val, torch.Tensor) or val.dtype != torch.float32:
            raise TypeError("val must be a torch.float32 tensor or None")
        if val.dim() != 1 or (not val_full and int(val.numel()) != blk.num_edges):
            raise ValueError("val must be 1-D%s, got %s" % ("" if val_full else " with one value per edge of the block: [%d]" % blk.num_edges,
                                                             tuple(val.shape)))
    for name, w in (("w1", w1), ("w2", w2)):
        if not isinstance(w, torch.Tensor) or w.dtype != x.dtype:
            raise TypeError("%s must be a tensor of x's dtype %s, got %s" % (name, x.dtype, getattr(w, "dtype", type(w).__name__)))
    if w1.dim() != 2 or int(w1.shape[0]) != feat or int(w1.shape[1]) < 1:
        raise ValueError("w1 must be [%d, hidden] with hidden >= 1, got %s" % (feat, tuple(w1.shape)))
    hidden = int(w1.shape[1])
    if w2.dim() != 2 or int(w2.shape[0]) != hidden or int(w2.shape[1]) < 1:
        raise ValueError("w2 must be [%d, n_out] with n_out >= 1, got %s" % (hidden, tuple(w2.shape)))
    n_out = int(w2.shape[1])
    shape = (blk.num_dst, n_out)
    for name, b, n in (("b1", b1, hidden), ("b2", b2, n_out)):
        if b is None:
            continue
        if not isinstance(b, torch.Tensor) or b.dtype != torch.float32:
            raise TypeError("%s must be a torch.float32 tensor or None" % name)
        if tuple(b.shape) != (n,):
            raise ValueError("%s must be [%d], got %s" % (name, n, tuple(b.shape)))
    if out is not None:
        _feat_dtype(out, "out")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError("out is %s, out_dtype says %s" % (out.dtype, out_dtype))
        if tuple(out.shape) != shape:
            raise ValueError("out must be [%d, %d], got %s" % (shape + (tuple(out.shape),)))
    odt = out.dtype if out is not None else (out_dtype or x.dtype)
    if x.dtype == torch.float32 and odt != torch.float32:
        raise TypeError("out_dtype: float32 operands give a float32 out, got %s" % (odt,))
    if fused and not block_gin_supported(feat, hidden, n_out, x.dtype):
        raise ValueError("fused=True: gnnagg_block_gin_supported(feat=%d, hidden=%d, n_out=%d, %s) says no" % (feat, hidden, n_out, x.dtype))
    # device tensors, contiguous where the call wants them dense
    px, pitch = _dev_ptr_rows(x, x.dtype, "x")
    p_ptr, p_idx = _dev_ptr(blk.ptr, torch.int32, "blk.ptr"), _dev_ptr(blk.idx, torch.int32, "blk.idx")
    p_src = _dev_ptr(blk.src_nodes, torch.int32, "blk.src_nodes") if mapped else None
    p_eid = _dev_ptr(blk.eid, torch.int32, "blk.eid") if val_full else None
    p_val = _dev_ptr(val, torch.float32, "val")
    p_w1, p_w2 = _dev_ptr(w1, x.dtype, "w1"), _dev_ptr(w2, x.dtype, "w2")
    p_b1, p_b2 = _dev_ptr(b1, torch.float32, "b1"), _dev_ptr(b2, torch.float32, "b2")
    if out is not None:
        _dev_ptr(out, out.dtype, "out")
    for name, t in (("blk.ptr", blk.ptr), ("val", val), ("w1", w1), ("w2", w2), ("b1", b1), ("b2", b2), ("out", out)):
        if t is not None and t.device != x.device:
            raise ValueError("%s lives on %s, x on %s" % (name, t.device, x.device))
    # ---- device work
    if fused is None:
        fused = gin_prefers_fused(blk.num_dst, feat, hidden, n_out, x.dtype)
    if not fused:   # the composition a caller writes with the existing calls
        if mapped:
            y, x_dst = block_gcn_run(blk, x, reduce=reduce, val=val, val_full=val_full, return_dst=True)
        else:
            y, x_dst = block_gcn_run(blk, x, reduce=reduce, val=val, val_full=val_full, gathered=gathered), x[:blk.num_dst]
        h = y + x_dst * self_scale      # a product, then a sum, each rounded to x's dtype (not add(alpha=): that is one fma)
        z = matmul_NN(h, w1, out_dtype=torch.float32)
        if b1 is not None:
            z = z + b1
        z = z.clamp_min(0).to(x.dtype)
        res = matmul_NN(z, w2, out_dtype=torch.float32)
        if b2 is not None:
            res = res + b2
        if relu:
            res = res.clamp_min(0)
        if out is None:
            return res.to(odt)
        out.copy_(res)
        return out
    if out is None:
        out = torch.empty(shape, dtype=odt, device=x.device)
    check(lib().gnnagg_block_gin_run(p_ptr, p_idx if blk.num_edges else None, blk.num_dst, p_src, p_val, p_eid, px, xdt, pitch, feat, self_scale,
                                     p_w1, p_b1, hidden, p_w2, p_b2, n_out, ctypes.c_void_p(out.data_ptr()) if blk.num_dst else None,
                                     FEATURE_DTYPES[out.dtype], REDUCE[reduce], _lib.FLAG_RELU if relu else 0,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


EDGECONV_COMBINES = {"diff": _lib.EDGECONV_DIFF, "cat": _lib.EDGECONV_CAT}


def block_edgeconv_supported(combine, feat, hidden, n_out, dtype):
    """gnnagg_block_edgeconv_supported: does the fused kernel of Block.edgeconv serve [2 feat] -> [hidden] -> [n_out] with operands of `dtype`?"""
    return (combine in EDGECONV_COMBINES and dtype in FEATURE_DTYPES
            and bool(lib().gnnagg_block_edgeconv_supported(EDGECONV_COMBINES[combine], int(feat), int(hidden), int(n_out), FEATURE_DTYPES[dtype])))


def edgeconv_prefers_fused(num_dst, combine, feat, hidden, n_out, dtype):
    """The fused=None rule of Block.edgeconv: the kernel wherever it is supported.  Its slowest round beat the composition's fastest
    round at all 64 shapes timed (profiles/block_edgeconv/README.md: arxiv- and products-shaped input blocks of 1 024 / 8 192 seeds and
    fanout 10 / 25, F = 3 and 64, hidden = n_out = 64, float32 and bfloat16, max and mean, combine="diff"; 1.33 - 4.58 x); no class
    lost.  "cat" and other widths were not timed and are taken with the measured ones."""
    return block_edgeconv_supported(combine, feat, hidden, n_out, dtype)


def block_edgeconv_run(blk, x, w1, w2, b1=None, b2=None, combine="diff", reduce="max", gathered=False, out=None, out_dtype=None, relu=False,
                       fused=None):
    """Block.edgeconv as a function (the thin form over gnnagg_block_edgeconv_run); every dtype and shape refusal is raised before device work"""
    if reduce not in REDUCE:
        raise ValueError("reduce must be one of %s, got %r" % (sorted(REDUCE), reduce))
    if combine not in EDGECONV_COMBINES:
        raise ValueError("combine must be one of %s, got %r" % (sorted(EDGECONV_COMBINES), combine))
    mapped = blk.src_nodes is not None and not gathered
    if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
        raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
    # types and shapes
    xdt = _feat_dtype(x, "x")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be 2-D [rows, F] with F >= 1, got %s" % (tuple(x.shape),))
    feat = int(x.shape[1])
    need_rows = max(blk.num_src, blk.num_dst) if not mapped else 0
    if int(x.shape[0]) < need_rows:
        raise ValueError("x has %d rows, the block's ids index %d (gathered=%s)" % (x.shape[0], need_rows, bool(gathered)))
    for name, w in (("w1", w1), ("w2", w2)):
        if not isinstance(w, torch.Tensor) or w.dtype != x.dtype:
            raise TypeError("%s must be a tensor of x's dtype %s, got %s" % (name, x.dtype, getattr(w, "dtype", type(w).__name__)))
    if w1.dim() != 2 or int(w1.shape[0]) != 2 * feat or int(w1.shape[1]) < 1:
        raise ValueError("w1 must be [%d, hidden] with hidden >= 1 (2 F rows: both halves of the message input), got %s" % (2 * feat, tuple(w1.shape)))
    hidden = int(w1.shape[1])
    if w2.dim() != 2 or int(w2.shape[0]) != hidden or int(w2.shape[1]) < 1:
        raise ValueError("w2 must be [%d, n_out] with n_out >= 1, got %s" % (hidden, tuple(w2.shape)))
    n_out = int(w2.shape[1])
    shape = (blk.num_dst, n_out)
    for name, b, n in (("b1", b1, hidden), ("b2", b2, n_out)):
        if b is None:
            continue
        if not isinstance(b, torch.Tensor) or b.dtype != torch.float32:
            raise TypeError("%s must be a torch.float32 tensor or None" % name)
        if tuple(b.shape) != (n,):
            raise ValueError("%s must be [%d], got %s" % (name, n, tuple(b.shape)))
    if out is not None:
        _feat_dtype(out, "out")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError("out is %s, out_dtype says %s" % (out.dtype, out_dtype))
        if tuple(out.shape) != shape:
            raise ValueError("out must be [%d, %d], got %s" % (shape + (tuple(out.shape),)))
    odt = out.dtype if out is not None else (out_dtype or x.dtype)
    if x.dtype == torch.float32 and odt != torch.float32:
        raise TypeError("out_dtype: float32 operands give a float32 out, got %s" % (odt,))
    if fused and not block_edgeconv_supported(combine, feat, hidden, n_out, x.dtype):
        raise ValueError("fused=True: gnnagg_block_edgeconv_supported(%s, feat=%d, hidden=%d, n_out=%d, %s) says no"
                         % (combine, feat, hidden, n_out, x.dtype))
    # device tensors, contiguous where the call wants them dense
    px, pitch = _dev_ptr_rows(x, x.dtype, "x")
    p_ptr, p_idx = _dev_ptr(blk.ptr, torch.int32, "blk.ptr"), _dev_ptr(blk.idx, torch.int32, "blk.idx")
    p_src = _dev_ptr(blk.src_nodes, torch.int32, "blk.src_nodes") if mapped else None
    p_w1, p_w2 = _dev_ptr(w1, x.dtype, "w1"), _dev_ptr(w2, x.dtype, "w2")
    p_b1, p_b2 = _dev_ptr(b1, torch.float32, "b1"), _dev_ptr(b2, torch.float32, "b2")
    if out is not None:
        _dev_ptr(out, out.dtype, "out")
    for name, t in (("blk.ptr", blk.ptr), ("w1", w1), ("w2", w2), ("b1", b1), ("b2", b2), ("out", out)):
        if t is not None and t.device != x.device:
            raise ValueError("%s lives on %s, x on %s" % (name, t.device, x.device))
    # ---- device work
    if fused is None:
        fused = edgeconv_prefers_fused(blk.num_dst, combine, feat, hidden, n_out, x.dtype)
    if not fused:   # the composition a caller writes with the existing calls
        E = blk.num_edges
        if E:
            rows = torch.searchsorted(blk.ptr[1:].long().contiguous(), torch.arange(E, device=x.device), right=True)
            ri, rs = (blk.src_nodes[rows].long(), blk.src_nodes[blk.idx.long()].long()) if mapped else (rows, blk.idx.long())
            xi, xs = x[ri], x[rs]
            z = matmul_NN(torch.cat([xi, xs - xi if combine == "diff" else xs], 1), w1, out_dtype=torch.float32)
            if b1 is not None:
                z = z + b1
            msg = matmul_NN(z.clamp_min(0).to(x.dtype), w2, out_dtype=torch.float32)
            if b2 is not None:
                msg = msg + b2
            edges = Block(blk.ptr, torch.arange(E, device=x.device, dtype=torch.int32), None, None, blk.num_dst, E, E)
            res = block_gcn_run(edges, msg, reduce=reduce, gathered=True)
        else:
            res = torch.zeros(shape, dtype=torch.float32, device=x.device)
        if relu:
            res = res.clamp_min(0)
        if out is None:
            return res.to(odt)
        out.copy_(res)
        return out
    if out is None:
        out = torch.empty(shape, dtype=odt, device=x.device)
    check(lib().gnnagg_block_edgeconv_run(p_ptr, p_idx if blk.num_edges else None, blk.num_dst, p_src, px, xdt, pitch, feat,
                                          EDGECONV_COMBINES[combine], p_w1, p_b1, hidden, p_w2, p_b2, n_out,
                                          ctypes.c_void_p(out.data_ptr()) if blk.num_dst else None, FEATURE_DTYPES[out.dtype], REDUCE[reduce],
                                          _lib.FLAG_RELU if relu else 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def block_pna_supported(feat, n_out, n_aggr, n_scaler, dtype):
    """gnnagg_block_pna_supported: does the fused kernel of Block.pna serve [feat] -> [n_out] with n_aggr aggregates x n_scaler scalers and
    operands of `dtype`?"""
    return dtype in FEATURE_DTYPES and bool(lib().gnnagg_block_pna_supported(int(feat), int(n_out), int(n_aggr), int(n_scaler),
                                                                             FEATURE_DTYPES[dtype]))


def pna_prefers_fused(num_dst, feat, n_out, n_aggr, n_scaler, dtype):
    """The fused=None rule of Block.pna: the kernel wherever it is supported.  (profiles/block_pna/rule_measurements.txt: the shapes
    measured and what each arm took.)"""
    return block_pna_supported(feat, n_out, n_aggr, n_scaler, dtype)


def block_pna_run(blk, x, w, w_self=None, bias=None, aggrs=("mean", "min", "max", "std"), scalers=("identity",), delta=None, val=None,
                  val_full=False, gathered=False, out=None, out_dtype=None, relu=False, fused=None):
    """Block.pna as a function (the thin form over gnnagg_block_pna_run); every dtype and shape refusal is raised before device work"""
    aggrs = (aggrs,) if isinstance(aggrs, str) else tuple(aggrs)
    scalers = (scalers,) if isinstance(scalers, str) else tuple(scalers)
    for names, table, what in ((aggrs, AGGRS, "aggrs"), (scalers, SCALERS, "scalers")):   # run_multi's validation and mask order
        if [n for n in names if n not in table] or not names or len(set(names)) != len(names):
            raise ValueError("%s must be distinct names of %s, got %r" % (what, sorted(table, key=table.get), names))
    amask, smask = sum(AGGRS[n] for n in aggrs), sum(SCALERS[n] for n in scalers)
    if smask != _lib.SCALER_IDENTITY:
        if delta is None:
            raise ValueError("the amplification and attenuation scalers need delta (pna_delta(ptr))")
        if not (math.isfinite(float(delta)) and float(delta) > 0.0):
            raise ValueError("delta = %r must be finite and > 0" % (delta,))
    mapped = blk.src_nodes is not None and not gathered
    if val_full and blk.eid is None:
        raise ValueError("val_full=True reads val through blk.eid: sample the block with return_eid=True")
    if val_full and val is None:
        raise ValueError("val_full=True needs val")
    if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
        raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
    # types and shapes
    xdt = _feat_dtype(x, "x")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be 2-D [rows, F] with F >= 1, got %s" % (tuple(x.shape),))
    feat = int(x.shape[1])
    need_rows = blk.num_src if not mapped else 0
    if w_self is not None and not mapped:
        need_rows = max(need_rows, blk.num_dst)
    if int(x.shape[0]) < need_rows:
        raise ValueError("x has %d rows, the block's ids index %d (gathered=%s)" % (x.shape[0], need_rows, bool(gathered)))
    if val is not None:
        if not isinstance(val, torch.Tensor) or val.dtype != torch.float32:
            raise TypeError("val must be a torch.float32 tensor or None")
        if val.dim() != 1 or (not val_full and int(val.numel()) != blk.num_edges):
            raise ValueError("val must be 1-D%s, got %s" % ("" if val_full else " with one value per edge of the block: [%d]" % blk.num_edges,
                                                             tuple(val.shape)))
    k_m = len(scalers) * len(aggrs) * feat
    for name, t, rows in (("w", w, k_m), ("w_self", w_self, feat)):
        if t is None and name == "w_self":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != x.dtype:
            raise TypeError("%s must be a tensor of x's dtype %s, got %s" % (name, x.dtype, getattr(t, "dtype", type(t).__name__)))
        if t.dim() != 2 or int(t.shape[0]) != rows or int(t.shape[1]) < 1 or t.shape[1] != w.shape[1]:
            raise ValueError("%s must be [%s = %d, n_out] with n_out >= 1%s, got %s" % (name, "S * A * F" if t is w else "F", rows,
                                                                                      "" if t is w else " as w's", tuple(t.shape)))
    n_out = int(w.shape[1])
    shape = (blk.num_dst, n_out)
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
            raise TypeError("bias must be a torch.float32 tensor or None")
        if tuple(bias.shape) != (n_out,):
            raise ValueError("bias must be [%d], got %s" % (n_out, tuple(bias.shape)))
    if out is not None:
        _feat_dtype(out, "out")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError("out is %s, out_dtype says %s" % (out.dtype, out_dtype))
        if tuple(out.shape) != shape:
            raise ValueError("out must be [%d, %d], got %s" % (shape + (tuple(out.shape),)))
    odt = out.dtype if out is not None else (out_dtype or x.dtype)
    if x.dtype == torch.float32 and odt != torch.float32:
        raise TypeError("out_dtype: float32 operands give a float32 out, got %s" % (odt,))
    if fused and not block_pna_supported(feat, n_out, len(aggrs), len(scalers), x.dtype):
        raise ValueError("fused=True: gnnagg_block_pna_supported(feat=%d, n_out=%d, n_aggr=%d, n_scaler=%d, %s) says no"
                         % (feat, n_out, len(aggrs), len(scalers), x.dtype))
    # device tensors, contiguous where the call wants them dense
    px, pitch = _dev_ptr_rows(x, x.dtype, "x")
    p_ptr, p_idx = _dev_ptr(blk.ptr, torch.int32, "blk.ptr"), _dev_ptr(blk.idx, torch.int32, "blk.idx")
    p_src = _dev_ptr(blk.src_nodes, torch.int32, "blk.src_nodes") if mapped else None
    p_eid = _dev_ptr(blk.eid, torch.int32, "blk.eid") if val_full else None
    p_val = _dev_ptr(val, torch.float32, "val")
    p_w, p_ws, p_b = _dev_ptr(w, x.dtype, "w"), _dev_ptr(w_self, x.dtype, "w_self"), _dev_ptr(bias, torch.float32, "bias")
    if out is not None:
        _dev_ptr(out, out.dtype, "out")
    for name, t in (("blk.ptr", blk.ptr), ("val", val), ("w", w), ("w_self", w_self), ("bias", bias), ("out", out)):
        if t is not None and t.device != x.device:
            raise ValueError("%s lives on %s, x on %s" % (name, t.device, x.device))
    # ---- device work
    if fused is None:
        fused = pna_prefers_fused(blk.num_dst, feat, n_out, len(aggrs), len(scalers), x.dtype)
    if not fused:   # the composition a caller writes with the existing calls
        x_src = x[blk.src_nodes.long()] if mapped else x.contiguous()
        m = torch.empty((blk.num_dst, k_m), dtype=x.dtype, device=x.device)
        h = blk.gcn(val[blk.eid.long()] if val_full else val)
        try:
            h.run_multi(x_src, m, aggrs=aggrs, scalers=scalers, delta=delta)
        finally:
            h.close()
        if w_self is not None:
            res = matmul_NN(torch.cat([x_src[:blk.num_dst], m], 1), torch.cat([w_self, w], 0), out_dtype=torch.float32)
        else:
            res = matmul_NN(m, w, out_dtype=torch.float32)
        if bias is not None:
            res = res + bias
        if relu:
            res = res.clamp_min(0)
        if out is None:
            return res.to(odt)
        out.copy_(res)
        return out
    if out is None:
        out = torch.empty(shape, dtype=odt, device=x.device)
    check(lib().gnnagg_block_pna_run(p_ptr, p_idx if blk.num_edges else None, blk.num_dst, p_src, p_val, p_eid, px, xdt, pitch, feat, amask, smask,
                                     ctypes.c_float(1.0 if delta is None else float(delta)), p_ws, p_w, p_b, n_out,
                                     ctypes.c_void_p(out.data_ptr()) if blk.num_dst else None, FEATURE_DTYPES[out.dtype],
                                     _lib.FLAG_RELU if relu else 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


RGCN_REDUCE = ("sum", "mean")


def block_rgcn_supported(feat, n_out, num_rel, dtype):
    """gnnagg_block_rgcn_supported: does the fused kernel of Block.rgcn serve [feat] -> [n_out] over num_rel relations with operands of `dtype`?"""
    return dtype in FEATURE_DTYPES and bool(lib().gnnagg_block_rgcn_supported(int(feat), int(n_out), int(num_rel), FEATURE_DTYPES[dtype]))


def rgcn_prefers_fused(num_dst, feat, n_out, num_rel, dtype):
    """The fused=None rule of Block.rgcn: the kernel wherever it is supported.  (profiles/block_rgcn/rule_measurements.txt: the shapes
    measured and what each arm took.)"""
    return block_rgcn_supported(feat, n_out, num_rel, dtype)


def _relation_block(blk, row_of_edge, keep):
    """the sub-block of the edges `keep` marks, in CSR order (a stable filter): what the composition of Block.rgcn aggregates per relation"""
    deg = torch.bincount(row_of_edge[keep], minlength=blk.num_dst)
    ptr = torch.zeros(blk.num_dst + 1, dtype=torch.int32, device=blk.ptr.device)
    ptr[1:] = deg.cumsum(0)
    idx = blk.idx[keep].contiguous()
    return Block(ptr, idx, blk.src_nodes, None, blk.num_dst, blk.num_src, int(idx.numel()))


def block_rgcn_run(blk, x, w_rel, etype, w_self=None, bias=None, reduce="mean", etype_full=False, val=None, val_full=False, gathered=False,
                   out=None, out_dtype=None, relu=False, fused=None):
    """Block.rgcn as a function (the thin form over gnnagg_block_rgcn_run); every dtype and shape refusal is raised before device work"""
    if reduce not in RGCN_REDUCE:
        raise ValueError("reduce must be one of %s, got %r" % (list(RGCN_REDUCE), reduce))
    mapped = blk.src_nodes is not None and not gathered
    for flag, name, t in ((etype_full, "etype", etype), (val_full, "val", val)):
        if flag and blk.eid is None:
            raise ValueError("%s_full=True reads %s through blk.eid: sample the block with return_eid=True" % (name, name))
        if flag and t is None:
            raise ValueError("%s_full=True needs %s" % (name, name))
    if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
        raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
    # types and shapes
    xdt = _feat_dtype(x, "x")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be 2-D [rows, F] with F >= 1, got %s" % (tuple(x.shape),))
    feat = int(x.shape[1])
    need_rows = blk.num_src if not mapped else 0
    if w_self is not None and not mapped:
        need_rows = max(need_rows, blk.num_dst)
    if int(x.shape[0]) < need_rows:
        raise ValueError("x has %d rows, the block's ids index %d (gathered=%s)" % (x.shape[0], need_rows, bool(gathered)))
    if not isinstance(etype, torch.Tensor) or etype.dtype != torch.int32:
        raise TypeError("etype must be a torch.int32 tensor, got %s" % (getattr(etype, "dtype", type(etype).__name__),))
    if etype.dim() != 1 or (not etype_full and int(etype.numel()) != blk.num_edges):
        raise ValueError("etype must be 1-D%s, got %s" % ("" if etype_full else " with one type per edge of the block: [%d]" % blk.num_edges,
                                                           tuple(etype.shape)))
    if val is not None:
        if not isinstance(val, torch.Tensor) or val.dtype != torch.float32:
            raise TypeError("val must be a torch.float32 tensor or None")
        if val.dim() != 1 or (not val_full and int(val.numel()) != blk.num_edges):
            raise ValueError("val must be 1-D%s, got %s" % ("" if val_full else " with one value per edge of the block: [%d]" % blk.num_edges,
                                                             tuple(val.shape)))
    if not isinstance(w_rel, torch.Tensor) or w_rel.dtype != x.dtype:
        raise TypeError("w_rel must be a tensor of x's dtype %s, got %s" % (x.dtype, getattr(w_rel, "dtype", type(w_rel).__name__)))
    if w_rel.dim() != 3 or int(w_rel.shape[0]) < 1 or int(w_rel.shape[1]) != feat or int(w_rel.shape[2]) < 1:
        raise ValueError("w_rel must be [R, %d, n_out] with R >= 1 and n_out >= 1, got %s" % (feat, tuple(w_rel.shape)))
    num_rel, n_out = int(w_rel.shape[0]), int(w_rel.shape[2])
    if w_self is not None:
        if not isinstance(w_self, torch.Tensor) or w_self.dtype != x.dtype:
            raise TypeError("w_self must be a tensor of x's dtype %s, got %s" % (x.dtype, getattr(w_self, "dtype", type(w_self).__name__)))
        if tuple(w_self.shape) != (feat, n_out):
            raise ValueError("w_self must be [%d, %d], as a relation of w_rel, got %s" % (feat, n_out, tuple(w_self.shape)))
    shape = (blk.num_dst, n_out)
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
            raise TypeError("bias must be a torch.float32 tensor or None")
        if tuple(bias.shape) != (n_out,):
            raise ValueError("bias must be [%d], got %s" % (n_out, tuple(bias.shape)))
    if out is not None:
        _feat_dtype(out, "out")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError("out is %s, out_dtype says %s" % (out.dtype, out_dtype))
        if tuple(out.shape) != shape:
            raise ValueError("out must be [%d, %d], got %s" % (shape + (tuple(out.shape),)))
    odt = out.dtype if out is not None else (out_dtype or x.dtype)
    if x.dtype == torch.float32 and odt != torch.float32:
        raise TypeError("out_dtype: float32 operands give a float32 out, got %s" % (odt,))
    if fused and not block_rgcn_supported(feat, n_out, num_rel, x.dtype):
        raise ValueError("fused=True: gnnagg_block_rgcn_supported(feat=%d, n_out=%d, num_rel=%d, %s) says no" % (feat, n_out, num_rel, x.dtype))
    # device tensors, contiguous where the call wants them dense
    px, pitch = _dev_ptr_rows(x, x.dtype, "x")
    p_ptr, p_idx = _dev_ptr(blk.ptr, torch.int32, "blk.ptr"), _dev_ptr(blk.idx, torch.int32, "blk.idx")
    p_src = _dev_ptr(blk.src_nodes, torch.int32, "blk.src_nodes") if mapped else None
    p_eid = _dev_ptr(blk.eid, torch.int32, "blk.eid") if val_full or etype_full else None
    p_et, p_val = _dev_ptr(etype, torch.int32, "etype"), _dev_ptr(val, torch.float32, "val")
    p_wr, p_ws, p_b = _dev_ptr(w_rel, x.dtype, "w_rel"), _dev_ptr(w_self, x.dtype, "w_self"), _dev_ptr(bias, torch.float32, "bias")
    if out is not None:
        _dev_ptr(out, out.dtype, "out")
    for name, t in (("blk.ptr", blk.ptr), ("etype", etype), ("val", val), ("w_rel", w_rel), ("w_self", w_self), ("bias", bias), ("out", out)):
        if t is not None and t.device != x.device:
            raise ValueError("%s lives on %s, x on %s" % (name, t.device, x.device))
    # ---- device work
    if fused is None:
        fused = rgcn_prefers_fused(blk.num_dst, feat, n_out, num_rel, x.dtype)
    if not fused:   # the composition a caller writes with the existing calls: R filtered sub-blocks, R aggregations, a cat, a GEMM
        t_e = etype[blk.eid.long()] if etype_full else etype
        v_e = val[blk.eid.long()] if val_full else val
        row_of_edge = torch.searchsorted(blk.ptr[1:].long().contiguous(), torch.arange(blk.num_edges, device=x.device), right=True)
        parts = []
        for r in range(num_rel):
            keep = t_e == r
            sub = _relation_block(blk, row_of_edge, keep)
            y = block_gcn_run(sub, x, reduce=reduce, val=None if v_e is None else v_e[keep].contiguous(), gathered=gathered,
                              return_dst=mapped and w_self is not None and r == 0)
            if isinstance(y, tuple):
                y, x_dst = y
                parts.append(x_dst)
            elif w_self is not None and r == 0:
                parts.append(x[:blk.num_dst])
            parts.append(y)
        ws = [] if w_self is None else [w_self]
        res = matmul_NN(torch.cat(parts, 1), torch.cat(ws + list(w_rel.unbind(0)), 0), out_dtype=torch.float32)
        if bias is not None:
            res = res + bias
        if relu:
            res = res.clamp_min(0)
        if out is None:
            return res.to(odt)
        out.copy_(res)
        return out
    if out is None:
        out = torch.empty(shape, dtype=odt, device=x.device)
    has_e = blk.num_edges > 0
    if not int(etype.numel()):   # (an empty tensor has a null pointer and the call wants an address: one element nobody reads)
        p_et = _dev_ptr(torch.zeros(1, dtype=torch.int32, device=x.device), torch.int32, "etype")
    check(lib().gnnagg_block_rgcn_run(p_ptr, p_idx if has_e else None, blk.num_dst, p_src, p_et, p_eid if etype_full else None, p_val,
                                      p_eid if val_full else None, px, xdt, pitch, feat, p_ws, p_wr, num_rel, p_b, n_out,
                                      ctypes.c_void_p(out.data_ptr()) if blk.num_dst else None, FEATURE_DTYPES[out.dtype],
                                      REDUCE[reduce], _lib.FLAG_RELU if relu else 0,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


# bases a lane of the basis kernel accumulates in one pass over a row, by the lane's width in columns (basis_chunk, agg_block_rgcn_basis.hip)
RGCN_BASIS_CHUNK = {1: 16, 2: 16, 4: 16, 8: 8}


def block_rgcn_basis_supported(feat, n_out, num_rel, num_bases, dtype):
    """gnnagg_block_rgcn_basis_supported: does the fused kernel of Block.rgcn_basis serve [feat] -> [n_out] over num_rel relations and
    num_bases bases with operands of `dtype`?"""
    return dtype in FEATURE_DTYPES and bool(lib().gnnagg_block_rgcn_basis_supported(int(feat), int(n_out), int(num_rel), int(num_bases),
                                                                                    FEATURE_DTYPES[dtype]))


def rgcn_basis_prefers_fused(num_dst, feat, n_out, num_rel, num_bases, dtype):
    """The fused=None rule of Block.rgcn_basis: the kernel where it is supported and Block.rgcn's kernel does NOT serve the materialised
    [num_rel, feat, n_out] weights -- there it was 5 to 120 x faster than the per-relation composition at every measured shape.  Where
    Block.rgcn's kernel fits (few relations), einsum + that kernel was as fast or faster at most shapes (up to 8 x at 30 bases: the basis
    walk pays one pass per 16 bases) and is taken.  (profiles/block_rgcn_basis/rule_measurements.txt: the shapes measured and what each
    arm took.)"""
    return block_rgcn_basis_supported(feat, n_out, num_rel, num_bases, dtype) and not block_rgcn_supported(feat, n_out, num_rel, dtype)


def block_rgcn_basis_run(blk, x, bases, comp, etype, w_self=None, bias=None, reduce="mean", etype_full=False, val=None, val_full=False,
                         gathered=False, out=None, out_dtype=None, relu=False, fused=None):
    """Block.rgcn_basis as a function (the thin form over gnnagg_block_rgcn_basis_run); every dtype and shape refusal is raised before
    device work"""
    if reduce not in RGCN_REDUCE:
        raise ValueError("reduce must be one of %s, got %r" % (list(RGCN_REDUCE), reduce))
    mapped = blk.src_nodes is not None and not gathered
    for flag, name, t in ((etype_full, "etype", etype), (val_full, "val", val)):
        if flag and blk.eid is None:
            raise ValueError("%s_full=True reads %s through blk.eid: sample the block with return_eid=True" % (name, name))
        if flag and t is None:
            raise ValueError("%s_full=True needs %s" % (name, name))
    if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
        raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
    # types and shapes
    xdt = _feat_dtype(x, "x")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be 2-D [rows, F] with F >= 1, got %s" % (tuple(x.shape),))
    feat = int(x.shape[1])
    need_rows = blk.num_src if not mapped else 0
    if w_self is not None and not mapped:
        need_rows = max(need_rows, blk.num_dst)
    if int(x.shape[0]) < need_rows:
        raise ValueError("x has %d rows, the block's ids index %d (gathered=%s)" % (x.shape[0], need_rows, bool(gathered)))
    if not isinstance(etype, torch.Tensor) or etype.dtype != torch.int32:
        raise TypeError("etype must be a torch.int32 tensor, got %s" % (getattr(etype, "dtype", type(etype).__name__),))
    if etype.dim() != 1 or (not etype_full and int(etype.numel()) != blk.num_edges):
        raise ValueError("etype must be 1-D%s, got %s" % ("" if etype_full else " with one type per edge of the block: [%d]" % blk.num_edges,
                                                           tuple(etype.shape)))
    if val is not None:
        if not isinstance(val, torch.Tensor) or val.dtype != torch.float32:
            raise TypeError("val must be a torch.float32 tensor or None")
        if val.dim() != 1 or (not val_full and int(val.numel()) != blk.num_edges):
            raise ValueError("val must be 1-D%s, got %s" % ("" if val_full else " with one value per edge of the block: [%d]" % blk.num_edges,
                                                             tuple(val.shape)))
    if not isinstance(bases, torch.Tensor) or bases.dtype != x.dtype:
        raise TypeError("bases must be a tensor of x's dtype %s, got %s" % (x.dtype, getattr(bases, "dtype", type(bases).__name__)))
    if bases.dim() != 3 or int(bases.shape[0]) < 1 or int(bases.shape[1]) != feat or int(bases.shape[2]) < 1:
        raise ValueError("bases must be [B, %d, n_out] with B >= 1 and n_out >= 1, got %s" % (feat, tuple(bases.shape)))
    num_bases, n_out = int(bases.shape[0]), int(bases.shape[2])
    if not isinstance(comp, torch.Tensor) or comp.dtype != torch.float32:
        raise TypeError("comp must be a torch.float32 tensor, got %s" % (getattr(comp, "dtype", type(comp).__name__),))
    if comp.dim() != 2 or int(comp.shape[0]) < 1 or int(comp.shape[1]) != num_bases:
        raise ValueError("comp must be [R, %d] with R >= 1, one column per basis, got %s" % (num_bases, tuple(comp.shape)))
    num_rel = int(comp.shape[0])
    if w_self is not None:
        if not isinstance(w_self, torch.Tensor) or w_self.dtype != x.dtype:
            raise TypeError("w_self must be a tensor of x's dtype %s, got %s" % (x.dtype, getattr(w_self, "dtype", type(w_self).__name__)))
        if tuple(w_self.shape) != (feat, n_out):
            raise ValueError("w_self must be [%d, %d], as a basis of bases, got %s" % (feat, n_out, tuple(w_self.shape)))
    shape = (blk.num_dst, n_out)
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
            raise TypeError("bias must be a torch.float32 tensor or None")
        if tuple(bias.shape) != (n_out,):
            raise ValueError("bias must be [%d], got %s" % (n_out, tuple(bias.shape)))
    if out is not None:
        _feat_dtype(out, "out")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError("out is %s, out_dtype says %s" % (out.dtype, out_dtype))
        if tuple(out.shape) != shape:
            raise ValueError("out must be [%d, %d], got %s" % (shape + (tuple(out.shape),)))
    odt = out.dtype if out is not None else (out_dtype or x.dtype)
    if x.dtype == torch.float32 and odt != torch.float32:
        raise TypeError("out_dtype: float32 operands give a float32 out, got %s" % (odt,))
    if fused and not block_rgcn_basis_supported(feat, n_out, num_rel, num_bases, x.dtype):
        raise ValueError("fused=True: gnnagg_block_rgcn_basis_supported(feat=%d, n_out=%d, num_rel=%d, num_bases=%d, %s) says no" %
                         (feat, n_out, num_rel, num_bases, x.dtype))
    # device tensors, contiguous where the call wants them dense
    px, pitch = _dev_ptr_rows(x, x.dtype, "x")
    p_ptr, p_idx = _dev_ptr(blk.ptr, torch.int32, "blk.ptr"), _dev_ptr(blk.idx, torch.int32, "blk.idx")
    p_src = _dev_ptr(blk.src_nodes, torch.int32, "blk.src_nodes") if mapped else None
    p_eid = _dev_ptr(blk.eid, torch.int32, "blk.eid") if val_full or etype_full else None
    p_et, p_val = _dev_ptr(etype, torch.int32, "etype"), _dev_ptr(val, torch.float32, "val")
    p_v, p_c = _dev_ptr(bases, x.dtype, "bases"), _dev_ptr(comp, torch.float32, "comp")
    p_ws, p_b = _dev_ptr(w_self, x.dtype, "w_self"), _dev_ptr(bias, torch.float32, "bias")
    if out is not None:
        _dev_ptr(out, out.dtype, "out")
    for name, t in (("blk.ptr", blk.ptr), ("etype", etype), ("val", val), ("bases", bases), ("comp", comp), ("w_self", w_self), ("bias", bias),
                    ("out", out)):
        if t is not None and t.device != x.device:
            raise ValueError("%s lives on %s, x on %s" % (name, t.device, x.device))
    # ---- device work
    if fused is None:
        fused = rgcn_basis_prefers_fused(blk.num_dst, feat, n_out, num_rel, num_bases, x.dtype)
    if not fused:   # the route a caller had before this call: materialise W_rel, then Block.rgcn with its own rule
        w_rel = torch.einsum("rb,bfn->rfn", comp, bases.float()).to(x.dtype)
        return block_rgcn_run(blk, x, w_rel, etype, w_self=w_self, bias=bias, reduce=reduce, etype_full=etype_full, val=val, val_full=val_full,
                              gathered=gathered, out=out, out_dtype=out_dtype, relu=relu, fused=None)
    if out is None:
        out = torch.empty(shape, dtype=odt, device=x.device)
    has_e = blk.num_edges > 0
    if not int(etype.numel()):   # (an empty tensor has a null pointer and the call wants an address: one element nobody reads)
        p_et = _dev_ptr(torch.zeros(1, dtype=torch.int32, device=x.device), torch.int32, "etype")
    check(lib().gnnagg_block_rgcn_basis_run(p_ptr, p_idx if has_e else None, blk.num_dst, p_src, p_et, p_eid if etype_full else None, p_val,
                                            p_eid if val_full else None, px, xdt, pitch, feat, p_ws, p_v, p_c, num_rel, num_bases, p_b, n_out,
                                            ctypes.c_void_p(out.data_ptr()) if blk.num_dst else None, FEATURE_DTYPES[out.dtype],
                                            REDUCE[reduce], _lib.FLAG_RELU if relu else 0,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


ATTN_KINDS = {"dot": _lib.ATTN_DOT, "gatv2": _lib.ATTN_GATV2}


def block_attn_run(blk, q, k, v=None, kind="dot", a=None, heads=1, scale=None, slope=0.2, bias=None, bias_full=False, edge=None,
                   edge_full=False, gathered=False, out=None, out_dtype=None):
    """Block.attend as a function (the thin form over gnnagg_block_attn_run); every dtype and shape refusal is raised before device work"""
    if kind not in ATTN_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(ATTN_KINDS), kind))
    dot = kind == "dot"
    mapped = blk.src_nodes is not None and not gathered
    for flag, name, t in ((bias_full, "bias", bias), (edge_full, "edge", edge)):
        if flag and blk.eid is None:
            raise ValueError("%s_full=True reads %s through blk.eid: sample the block with return_eid=True" % (name, name))
        if flag and t is None:
            raise ValueError("%s_full=True needs %s" % (name, name))
    if bias is not None and edge is not None and bool(bias_full) != bool(edge_full):
        raise ValueError("bias and edge are both per edge of the block or both per edge of the full CSR (one eid serves both)")
    if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
        raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
    if dot and v is None:
        raise ValueError("kind='dot' needs v (the rows to sum)")
    if not dot and v is not None:
        raise ValueError("kind='gatv2' sums the rows it scores (k): v must be None")
    if dot and a is not None:
        raise ValueError("kind='dot' takes no a")
    # types and shapes
    xdt = _feat_dtype(q, "q")
    ops = (("q", q), ("k", k)) + ((("v", v),) if dot else ())
    for name, t in ops[1:]:
        if _feat_dtype(t, name) != xdt:
            raise TypeError("%s (%s) must have q's dtype %s" % (name, t.dtype, q.dtype))
    for name, t in ops:
        if t.dim() != 2 or t.shape[1] < 1:
            raise ValueError("%s must be 2-D [rows, F] with F >= 1, got %s" % (name, tuple(t.shape)))
    feat, heads = int(q.shape[1]), int(heads)
    if heads < 1 or feat % heads != 0:
        raise ValueError("heads = %d does not divide F = %d" % (heads, feat))
    if feat > Aggregator_GAT.GATV2_MAX_FEAT:
        raise ValueError("F = %d is above the kernel's limit of %d columns" % (feat, Aggregator_GAT.GATV2_MAX_FEAT))
    for name, t in ops[1:]:
        if int(t.shape[1]) != feat:
            raise ValueError("%s has %d columns, q has %d" % (name, t.shape[1], feat))
    if dot and (tuple(k.shape) != tuple(v.shape) or (k.shape[0] > 1 and k.stride(0) != v.stride(0))):
        raise ValueError("k %s and v %s must have one shape and share one row pitch (stride(0) = %d and %d)" %
                         (tuple(k.shape), tuple(v.shape), k.stride(0), v.stride(0)))
    if not mapped and (int(k.shape[0]) < blk.num_src or int(q.shape[0]) < blk.num_dst):
        raise ValueError("q has %d rows and k %d, the block's ids index %d and %d (gathered=%s)" %
                         (q.shape[0], k.shape[0], blk.num_dst, blk.num_src, bool(gathered)))
    if not dot:
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float32:
            raise TypeError("kind='gatv2' needs a: a torch.float32 tensor of heads * D elements")
        if int(a.numel()) != feat:
            raise ValueError("a %s does not hold [heads = %d, D = %d]" % (tuple(a.shape), heads, feat // heads))
        if not 0.0 <= float(slope) <= 1.0:
            raise ValueError("slope = %r is outside [0, 1]" % (slope,))
    scale = 1.0 / math.sqrt(feat // heads) if scale is None else float(scale)
    if not math.isfinite(scale) or not math.isfinite(ctypes.c_float(scale).value):
        raise ValueError("scale = %r is not finite (in fp32)" % (scale,))
    bias_heads = 1
    if bias is not None:
        bias_heads = _bias_heads(bias, int(bias.shape[0]) if bias_full and isinstance(bias, torch.Tensor) and bias.dim() else blk.num_edges, heads,
                                 q, "Block.attend")
    ef = None
    if edge is not None:
        ef = _edge_rows(edge, int(edge.shape[0]) if edge_full and isinstance(edge, torch.Tensor) and edge.dim() else blk.num_edges, feat, q,
                        "Block.attend")
    shape = (blk.num_dst, feat)
    if out is not None:
        _feat_dtype(out, "out")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError("out is %s, out_dtype says %s" % (out.dtype, out_dtype))
        if tuple(out.shape) != shape:
            raise ValueError("out must be [%d, %d], got %s" % (shape + (tuple(out.shape),)))
    # device tensors, contiguous where the call wants them dense
    (pq, q_pitch), (pk, kv_pitch) = _dev_ptr_rows(q, q.dtype, "q"), _dev_ptr_rows(k, k.dtype, "k")
    pv = _dev_ptr_rows(v, v.dtype, "v")[0] if dot else None
    p_ptr, p_idx = _dev_ptr(blk.ptr, torch.int32, "blk.ptr"), _dev_ptr(blk.idx, torch.int32, "blk.idx")
    p_src = _dev_ptr(blk.src_nodes, torch.int32, "blk.src_nodes") if mapped else None
    p_eid = _dev_ptr(blk.eid, torch.int32, "blk.eid") if bias_full or edge_full else None
    p_a, p_bias = _dev_ptr(a, torch.float32, "a"), _dev_ptr(bias, torch.float32, "bias")
    if out is not None:
        _dev_ptr(out, out.dtype, "out")
    for name, t in ops[1:] + (("blk.ptr", blk.ptr), ("a", a), ("out", out)):
        if t is not None and t.device != q.device:
            raise ValueError("%s lives on %s, q on %s" % (name, t.device, q.device))
    # ---- device work
    if out is None:
        out = torch.empty(shape, dtype=out_dtype or q.dtype, device=q.device)
    has_e = blk.num_edges > 0
    check(lib().gnnagg_block_attn_run(p_ptr, p_idx if has_e else None, blk.num_dst, p_src, p_eid if has_e else None, ATTN_KINDS[kind], pq, q_pitch, pk, pv, kv_pitch,
                                      p_a, ctypes.c_float(slope), ctypes.c_float(scale), p_bias if has_e else None, bias_heads,
                                      ef[0] if ef is not None and has_e else None, ef[1] if ef is not None else 0, xdt,
                                      ctypes.c_void_p(out.data_ptr()) if blk.num_dst else None, FEATURE_DTYPES[out.dtype], feat, heads,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def _check_fanout(fanout):
    fanout = int(fanout)
    if fanout == 0 or fanout < -1:
        raise ValueError("fanout must be -1 (every edge) or >= 1, got %d" % fanout)
    return fanout


class NeighborSampler:
    """gnnagg_sampler over a device CSR (int32 tensors, kept alive by this object).  prob: None (uniform sampling) or one float32 weight
    per edge of the full CSR (device tensor [num_e], kept alive too): neighbours are drawn without replacement in proportion to it, and an
    edge whose weight is not > 0 is never kept (set_prob)."""

    def __init__(self, ptr, idx, prob=None):
        self.ptr, self.idx = ptr, idx
        self.prob = None
        self.num_v = int(ptr.numel()) - 1
        self.num_e = int(idx.numel())
        self._h = ctypes.c_int64(0)
        check(lib().gnnagg_sampler_create(_dev_ptr(ptr, torch.int32, "ptr"), _dev_ptr(idx, torch.int32, "idx"), self.num_v, self.num_e,
                                          ctypes.byref(self._h)))
        if prob is not None:
            self.set_prob(prob)

    def set_prob(self, prob):
        """gnnagg_sampler_set_weights: the per-edge weights of every later sample (None: uniform sampling again).  Checked by dtype and
        size only.  Counts every row's eligible edges once, on torch's current stream, and waits for it."""
        L = lib()
        if prob is None:
            check(L.gnnagg_sampler_set_weights(self._h, None))
            self.prob = None
            return
        p = _dev_ptr(prob, torch.float32, "prob")
        if prob.dim() != 1 or int(prob.numel()) != self.num_e:
            raise ValueError("prob must hold one weight per edge: [%d], got %s" % (self.num_e, tuple(prob.shape)))
        check(L.gnnagg_sampler_set_stream(self._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        check(L.gnnagg_sampler_set_weights(self._h, p))   # (a graph without edges: a null pointer, and nothing to weigh)
        self.prob = prob

    def close(self):
        if self._h.value:
            lib().gnnagg_sampler_destroy(self._h)
            self._h = ctypes.c_int64(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sample(self, seeds, fanout, seed=0, relabel=True, return_eid=False):
        """One block.  seeds: device int32 [n] (duplicates allowed).  The work goes to torch's current stream; reading the two counts
        back is the one synchronisation per block (fanout = -1 reads the seeds' degree sum first, to size the outputs)."""
        fanout = _check_fanout(fanout)
        _dev_ptr(seeds, torch.int32, "seeds")
        if seeds.dim() != 1:
            raise ValueError("seeds must be 1-D, got %s" % (tuple(seeds.shape),))
        n, dev = int(seeds.numel()), seeds.device
        if fanout > 0:
            cap = n * fanout
        else:
            sl = seeds.long()
            cap = int((self.ptr[sl + 1] - self.ptr[sl]).sum().item()) if n else 0
        if n + cap >= 1 << 31:
            raise ValueError("num_seeds + cap_e = %d does not stay below 2^31" % (n + cap))
        # (an empty tensor has a null pointer: every buffer holds one element at least)
        blk_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        blk_idx = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        eid = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if return_eid else None
        src = torch.empty(max(n + cap, 1), dtype=torch.int32, device=dev) if relabel else None
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        L = lib()
        check(L.gnnagg_sampler_set_stream(self._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        check(L.gnnagg_sampler_sample(self._h, ctypes.c_void_p(seeds.data_ptr()) if n else None, n, fanout, int(seed) & _U64,
                                      ctypes.c_void_p(blk_ptr.data_ptr()), ctypes.c_void_p(blk_idx.data_ptr()),
                                      ctypes.c_void_p(eid.data_ptr()) if return_eid else None, cap,
                                      ctypes.c_void_p(src.data_ptr()) if relabel else None, ctypes.c_void_p(counts.data_ptr())))
        num_edges, num_src = (int(v) for v in counts.tolist())
        if num_edges > cap:
            raise RuntimeError("sample: %d edges kept, room for %d (the CSR changed under the sampler?)" % (num_edges, cap))
        return Block(blk_ptr, blk_idx[:num_edges], src[:num_src] if relabel else None, eid[:num_edges] if return_eid else None, n, num_src,
                     num_edges)

    def sample_layers(self, seeds, fanouts=(15, 10), seed=0, return_eid=False):
        """Blocks of a len(fanouts)-layer network, INPUT layer first (fanouts[l] belongs to layer l).  Built from the output layer down:
        the block of layer l uses seed + l and takes the src_nodes of the block above it as its seeds, so blocks[l].num_dst ==
        blocks[l + 1].num_src and the features of blocks[0].src_nodes are what the forward pass loads."""
        blocks = [None] * len(fanouts)
        for l in range(len(fanouts) - 1, -1, -1):
            blocks[l] = self.sample(seeds, fanouts[l], seed=int(seed) + l, relabel=True, return_eid=return_eid)
            seeds = blocks[l].src_nodes
        return blocks


def sample_block_host(ptr, idx, seeds, fanout, seed=0, relabel=True, return_eid=False, prob=None):
    """gnnagg_sample_block_host: numpy int32 arrays in, a Block of numpy arrays out -- the device sampler's specification, bit for bit.
    prob: None or one float32 weight per edge (gnnagg_sample_block_host_weighted)."""
    fanout = _check_fanout(fanout)
    ptr, idx, seeds = (np.ascontiguousarray(a, dtype=np.int32) for a in (ptr, idx, seeds))
    if ptr.ndim != 1 or idx.ndim != 1 or seeds.ndim != 1 or ptr.size < 1:
        raise ValueError("ptr, idx and seeds must be 1-D, ptr with num_v + 1 entries")
    n, num_v = int(seeds.size), int(ptr.size) - 1
    if n and (seeds.min() < 0 or seeds.max() >= num_v):
        raise ValueError("a seed is no row of the graph")
    cap = n * fanout if fanout > 0 else int((ptr[seeds.astype(np.int64) + 1].astype(np.int64) - ptr[seeds]).sum())
    blk_ptr = np.empty(n + 1, np.int32)
    blk_idx = np.empty(max(cap, 1), np.int32)
    eid = np.empty(max(cap, 1), np.int32) if return_eid else None
    src = np.empty(max(n + cap, 1), np.int32) if relabel else None
    counts = np.zeros(2, np.int32)
    p = lambda a: None if a is None else a.ctypes.data
    if prob is None:
        check(lib().gnnagg_sample_block_host(p(ptr), p(idx), num_v, p(seeds), n, fanout, int(seed) & _U64, p(blk_ptr), p(blk_idx), p(eid), cap,
                                             p(src), p(counts)))
    else:
        prob = np.ascontiguousarray(prob, dtype=np.float32)
        if prob.ndim != 1 or prob.size != idx.size:
            raise ValueError("prob must hold one weight per edge: [%d], got %s" % (idx.size, prob.shape))
        if prob.size == 0:
            prob = np.zeros(1, np.float32)   # (an empty array has no address; no edge reads it)
        check(lib().gnnagg_sample_block_host_weighted(p(ptr), p(idx), p(prob), num_v, p(seeds), n, fanout, int(seed) & _U64, p(blk_ptr), p(blk_idx),
                                                      p(eid), cap, p(src), p(counts)))
    num_edges, num_src = int(counts[0]), int(counts[1])
    return Block(blk_ptr, blk_idx[:num_edges], src[:num_src] if relabel else None, eid[:num_edges] if return_eid else None, n, num_src, num_edges)
