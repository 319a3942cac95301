"""The contract of gnnagg_block_gcn_run (include/gnnagg.h section F, "Block aggregation") restated in numpy, and the synthetic block the
block-run tests share.  Written from the contract, not from the kernel: one loop over a row's edges in CSR order.

chain32 is the fp32 chain itself.  Without val it is exact: fmaf(x, 1, acc) is ONE rounded addition, which is what np.float32 + np.float32
is.  With val every step is float32(float64(x) * float64(w) + float64(acc)): the product is exact in float64, the sum is rounded twice, so
the result is the fused one wherever the float64 sum is exact (hand-worked examples in small dyadic numbers) and may differ in the last bit
elsewhere -- the GPU tests with val therefore take the handle's rows mode as the bit-for-bit yardstick and sum64 for the bound.
"""
import functools

import numpy as np

DEGREES = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300]   # every side of every GROUP and of the gather batch
NUM_SRC = 257        # source rows of the synthetic block (ids drawn with repeats)
NUM_X = 1000         # rows of the full feature matrix src_nodes points into
NUM_E_FULL = 5000    # edges of the (imagined) full CSR that eid points into


def _row_sources(ptr, idx, i, src_nodes):
    s = np.asarray(idx[int(ptr[i]):int(ptr[i + 1])], np.int64)
    return s if src_nodes is None else np.asarray(src_nodes, np.int64)[s]


def _row_weights(ptr, i, val, eid):
    p = np.arange(int(ptr[i]), int(ptr[i + 1]), dtype=np.int64)
    if val is None:
        return None
    return np.asarray(val, np.float32)[p if eid is None else np.asarray(eid, np.int64)[p]]


def chain32(ptr, idx, x, reduce, val=None, src_nodes=None, eid=None, relu=False):
    """y [num_dst, F] float32: the contract's chain.  x: float32 [rows, F] (a bf16 x is passed widened)."""
    x = np.asarray(x, np.float32)
    n, F = len(ptr) - 1, x.shape[1]
    y = np.zeros((n, F), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            s, w = _row_sources(ptr, idx, i, src_nodes), _row_weights(ptr, i, val, eid)
            if len(s) == 0:
                continue                                         # 0 for a row without edges, whatever the reduce
            if reduce == "max":
                acc = np.full(F, -np.inf, np.float32)
                for e in range(len(s)):
                    t = x[s[e]] if w is None else x[s[e]] * w[e]  # one rounded fp32 product (x * 1 is x)
                    acc = np.where(t > acc, t, acc)
            else:
                acc = np.zeros(F, np.float32)
                for e in range(len(s)):
                    if w is None:
                        acc = x[s[e]] + acc
                    else:
                        acc = (x[s[e]].astype(np.float64) * np.float64(w[e]) + acc.astype(np.float64)).astype(np.float32)
                if reduce == "mean":
                    acc = acc / np.float32(len(s))                # deg = the row's edges in the block
            y[i] = acc
        if relu:
            y = np.where(y < 0, np.float32(0), y)                 # a NaN stays a NaN
    return y


def sum64(ptr, idx, x, val=None, src_nodes=None, eid=None):
    """(float64 sum of w * x per row, sum of |w * x| per row): the value and the scale of the project's 1e-5 bound; mean = both / deg"""
    x = np.asarray(x, np.float64)
    n, F = len(ptr) - 1, x.shape[1]
    out, scale = np.zeros((n, F)), np.zeros((n, F))
    for i in range(n):
        s, w = _row_sources(ptr, idx, i, src_nodes), _row_weights(ptr, i, val, eid)
        if len(s):
            t = x[s] if w is None else x[s] * w.astype(np.float64)[:, None]
            out[i], scale[i] = t.sum(0), np.abs(t).sum(0)
    return out, scale


def degrees(ptr):
    return np.diff(np.asarray(ptr, np.int64))


@functools.lru_cache(maxsize=None)
def synthetic_block():
    """dict of int32 arrays: ptr / idx (rows of DEGREES, ids drawn with repeats from NUM_SRC source rows), src_nodes (a slice of a
    permutation of the NUM_X rows of x), eid (distinct positions in a full CSR of NUM_E_FULL edges, increasing inside a row as the
    sampler leaves them)"""
    rng = np.random.default_rng(20250101)
    ptr = np.concatenate([[0], np.cumsum(DEGREES)]).astype(np.int32)
    num_e = int(ptr[-1])
    idx = rng.integers(0, NUM_SRC, size=num_e).astype(np.int32)
    src_nodes = rng.permutation(NUM_X)[:NUM_SRC].astype(np.int32)
    eid = np.sort(rng.choice(NUM_E_FULL, num_e, replace=False)).astype(np.int32)
    return {"ptr": ptr, "idx": idx, "src_nodes": src_nodes, "eid": eid, "num_dst": len(DEGREES), "num_src": NUM_SRC, "num_edges": num_e}
