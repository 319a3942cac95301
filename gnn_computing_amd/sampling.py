"""Neighbour sampling (include/gnnagg.h section F): seeds + fanout -> a message-flow block, on the device (csrc/sample.hip) or the
host (csrc/host_graph.cpp).  The sample of a row is a function of (seed, the row's edge positions) alone: the same in every batch, on
either path, bit for bit.  Sampling is not capturable into a HIP graph (sizes are data-dependent and read back once per block).
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .aggregator import FEATURE_DTYPES, REDUCE, Aggregator_GAT, Aggregator_GCN, _dev_ptr, _dev_ptr_rows, _feat_dtype

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
