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
from .aggregator import Aggregator_GAT, Aggregator_GCN, _dev_ptr

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


def _check_fanout(fanout):
    fanout = int(fanout)
    if fanout == 0 or fanout < -1:
        raise ValueError("fanout must be -1 (every edge) or >= 1, got %d" % fanout)
    return fanout


class NeighborSampler:
    """gnnagg_sampler over a device CSR (int32 tensors, kept alive by this object)."""

    def __init__(self, ptr, idx):
        self.ptr, self.idx = ptr, idx
        self.num_v = int(ptr.numel()) - 1
        self.num_e = int(idx.numel())
        self._h = ctypes.c_int64(0)
        check(lib().gnnagg_sampler_create(_dev_ptr(ptr, torch.int32, "ptr"), _dev_ptr(idx, torch.int32, "idx"), self.num_v, self.num_e,
                                          ctypes.byref(self._h)))

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


def sample_block_host(ptr, idx, seeds, fanout, seed=0, relabel=True, return_eid=False):
    """gnnagg_sample_block_host: numpy int32 arrays in, a Block of numpy arrays out -- the device sampler's specification, bit for bit."""
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
    check(lib().gnnagg_sample_block_host(p(ptr), p(idx), num_v, p(seeds), n, fanout, int(seed) & _U64, p(blk_ptr), p(blk_idx), p(eid), cap, p(src),
                                         p(counts)))
    num_edges, num_src = int(counts[0]), int(counts[1])
    return Block(blk_ptr, blk_idx[:num_edges], src[:num_src] if relabel else None, eid[:num_edges] if return_eid else None, n, num_src, num_edges)
