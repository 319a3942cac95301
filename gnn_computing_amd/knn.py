"""k-nearest-neighbour graphs (include/gnnagg.h section I): for every query row the k closest candidates of its segment, as the (ptr, idx)
of a Block of global ids -- the graph a dynamic-graph layer (DGCNN: knn_graph + Block.edgeconv per layer) rebuilds in feature space.
One kernel (csrc/agg_knn.hip): distances on the MFMA, a streaming top-k selection, no [N, M] matrix in memory.
"""
import ctypes

import torch

from . import _lib
from ._lib import check, lib
from .aggregator import FEATURE_DTYPES, _dev_ptr, _dev_ptr_rows, _feat_dtype
from .sampling import Block

KNN_MAX_FEAT, KNN_MAX_K, KNN_MAX_SPLITS = 256, 64, 16


def knn_supported(feat, k, dtype):
    """gnnagg_knn_supported: does the kernel serve rows of `feat` elements of `dtype` and k neighbours?"""
    return dtype in FEATURE_DTYPES and bool(lib().gnnagg_knn_supported(int(feat), int(k), FEATURE_DTYPES[dtype]))


def knn_prefers_fused(n, m, feat, k, dtype):
    """The fused=None rule of knn_graph: the kernel wherever it is supported.  Its slowest round beat the composition's fastest at the
    10 shapes timed with the library's own splits (profiles/knn/README.md: 32 x 1 024 points with F = 3, 64, 128, 8 x 4 096, 1 x 2 048;
    float32 and bfloat16; 1.73 - 11.4 x).  With splits=1 forced on one cloud of 2 048 points the composition won (0.83 x, 0.90 x)."""
    return knn_supported(feat, k, dtype)


def knn_work_bytes(n, m, feat, k, dtype, num_seg=1, splits=0):
    """gnnagg_knn_work_bytes: the bytes of workspace a knn_run of this shape needs (0 where the candidate range is not split)"""
    nb = int(lib().gnnagg_knn_work_bytes(int(n), int(m), int(feat), int(k), FEATURE_DTYPES[dtype], int(num_seg), int(splits)))
    if nb < 0:
        raise ValueError(lib().gnnagg_last_error().decode())
    return nb


def knn_out_ptr(n, m, k, ptr=None, y_ptr=None, exclude_self=False):
    """ptr [n + 1] of the result, int32 on the segments' device: the running sum of count_i = min(k, candidates of the row's segment -
    (1 where the row itself is excluded)), a closed form of the segment sizes.  ptr / y_ptr: int32 [B + 1] or None (one segment)."""
    ex = 1 if exclude_self else 0
    if ptr is None:
        return torch.arange(n + 1, dtype=torch.int64) * max(min(k, m - ex), 0)
    yp = ptr if y_ptr is None else y_ptr
    per_seg = (yp[1:].long() - yp[:-1].long() - ex).clamp(0, k)
    counts = torch.repeat_interleave(per_seg, ptr[1:].long() - ptr[:-1].long(), output_size=n)
    return torch.cat([counts.new_zeros(1), counts.cumsum(0)])


def _check_segments(name, p, rows):
    """the host copy of a pointer tensor; ValueError unless it ascends from 0 to rows"""
    if not isinstance(p, torch.Tensor) or p.dtype != torch.int32 or p.dim() != 1 or p.numel() < 2:
        raise TypeError("%s must be a 1-D torch.int32 tensor of B + 1 >= 2 entries" % name)
    h = p.tolist()
    if h[0] != 0 or h[-1] != rows:
        raise ValueError("%s must run from 0 to %d, got %d .. %d" % (name, rows, h[0], h[-1]))
    if any(b < a for a, b in zip(h, h[1:])):
        raise ValueError("%s must ascend" % name)
    return h


def knn_run(x, k, out_ptr, idx, dist=None, ptr=None, y=None, y_ptr=None, loop=False, splits=0, work=None):
    """The thin form over gnnagg_knn_run on torch's current stream: no allocation (but `work` where it is None and needed), no host
    synchronisation, capturable.  out_ptr int32 [N + 1] (knn_out_ptr), idx int32 [out_ptr[N]], dist float32 of idx's length or None."""
    xdt = _feat_dtype(x, "x")
    px, xpitch = _dev_ptr_rows(x, x.dtype, "x")
    n, feat = int(x.shape[0]), int(x.shape[1])
    py, ypitch, m = None, 0, n
    if y is not None:
        py, ypitch = _dev_ptr_rows(y, x.dtype, "y")
        m = int(y.shape[0])
        if int(y.shape[1]) != feat:
            raise ValueError("y must be [M, %d] as x, got %s" % (feat, tuple(y.shape)))
    num_seg = int(ptr.numel()) - 1 if ptr is not None else 0
    p_xp = _dev_ptr(ptr, torch.int32, "ptr")
    p_yp = _dev_ptr(y_ptr if y_ptr is not None else ptr, torch.int32, "y_ptr") if y is not None else None
    if idx.numel() == 0:   # no row keeps a candidate (an empty tensor has no address to pass)
        return
    if work is None:
        nb =knn_work_bytes(n, m, feat, k, x.dtype, max(num_seg, 1), splits)
        work = torch.empty(nb, dtype=torch.uint8, device=x.device) if nb else None
    check(lib().gnnagg_knn_run(px, py, xdt, xpitch, ypitch, n, m, feat, int(k), p_xp, p_yp, num_seg, 1 if loop else 0,
                               _dev_ptr(out_ptr, torch.int32, "out_ptr"), _dev_ptr(idx, torch.int32, "idx"), _dev_ptr(dist, torch.float32, "dist"),
                               _dev_ptr(work, torch.uint8, "work"), int(work.numel()) if work is not None else 0, int(splits),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def knn_graph(x, k, ptr=None, y=None, y_ptr=None, loop=False, return_dist=False, splits=0, fused=None):
    """The k nearest candidates of every query, as a Block of global ids (Block.edgeconv, aggregate, attend, score ... take it as it is).
      x            float32 or bfloat16 [N, F] queries; a row-pitched column view (stride(1) == 1) is taken as it is
      y            None (the candidates are the queries) or [M, F] of x's dtype
      ptr, y_ptr   None (one segment) or int32 [B + 1] ascending from 0 to N / M, a `batch` vector in pointer form: a query sees the
                   candidates of its own segment only.  With y None, y_ptr is ptr.
      loop         y None only: False excludes j == i by index
      the order    per query the candidates ascending by (d_ij, j), d_ij = max(|x_i|^2 + |y_j|^2 - 2 x_i . y_j, 0) in float32 (bfloat16
                   rows widened exactly); ties go to the lower j; the first min(k, segment size - excluded) are kept in that order.
      fused        True: the kernel, ValueError where knn_supported says no (1 <= F <= 256, 1 <= k <= 64) or x is not on the device.
                   False: the torch composition per segment (norm expansion, stable sort, cut), CPU tensors too.  None: knn_prefers_fused.
      splits       0: the library chooses into how many shares a candidate range is cut; 1 .. 16: that many.  No bit depends on it.
    Returns Block(ptr [N + 1], idx [E], None, None, N, M, E), and dist float32 [E] behind it with return_dist."""
    _feat_dtype(x, "x")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be 2-D [N, F] with F >= 1, got %s" % (tuple(x.shape),))
    n, feat = int(x.shape[0]), int(x.shape[1])
    k = int(k)
    if k < 1:
        raise ValueError("k = %d must be >= 1" % k)
    if not 0 <= int(splits) <= KNN_MAX_SPLITS:
        raise ValueError("splits = %d lies outside 0..%d" % (splits, KNN_MAX_SPLITS))
    if y is None:
        if y_ptr is not None:
            raise ValueError("y_ptr is given without y")
        m = n
    else:
        if not isinstance(y, torch.Tensor) or y.dtype != x.dtype or y.dim() != 2 or int(y.shape[1]) != feat:
            raise TypeError("y must be a [M, %d] tensor of x's dtype %s" % (feat, x.dtype))
        if loop:
            raise ValueError("loop belongs to y=None: with candidates of their own no j is excluded")
        if (ptr is None) != (y_ptr is None):
            raise ValueError("ptr and y_ptr come together when y is given")
        m = int(y.shape[0])
    hx = _check_segments("ptr", ptr, n) if ptr is not None else [0, n]
    hy = hx if y is None else (_check_segments("y_ptr", y_ptr, m) if y_ptr is not None else [0, m])
    if len(hx) != len(hy):
        raise ValueError("ptr and y_ptr must name the same number of segments, got %d and %d" % (len(hx) - 1, len(hy) - 1))
    for name, t in (("ptr", ptr), ("y", y), ("y_ptr", y_ptr)):
        if t is not None and t.device != x.device:
            raise ValueError("%s lives on %s, x on %s" % (name, t.device, x.device))
    if fused and not (x.is_cuda and knn_supported(feat, k, x.dtype)):
        raise ValueError("fused=True: %s" % ("gnnagg_knn_supported(feat=%d, k=%d, %s) says no" % (feat, k, x.dtype) if x.is_cuda
                                             else "x must be a HIP device tensor"))
    if fused is None:
        fused = x.is_cuda and knn_prefers_fused(n, m, feat, k, x.dtype)
    excl = y is None and not loop
    out_ptr = knn_out_ptr(n, m, k, ptr, y_ptr, excl).to(device=x.device, dtype=torch.int32)
    num_e = sum((b - a) * max(min(k, d - c - (1 if excl else 0)), 0) for a, b, c, d in zip(hx, hx[1:], hy, hy[1:]))
    if fused:
        idx = torch.empty(num_e, dtype=torch.int32, device=x.device)
        dist = torch.empty(num_e, dtype=torch.float32, device=x.device) if return_dist else None
        if n:
            knn_run(x, k, out_ptr, idx, dist, ptr=ptr, y=y, y_ptr=y_ptr, loop=loop, splits=splits)
    else:   # the composition a caller writes with torch
        cand = x if y is None else y
        ids, ds = [], []
        for a, b, c, d in zip(hx, hx[1:], hy, hy[1:]):
            keep = max(min(k, d - c - (1 if excl else 0)), 0)
            if b == a or keep == 0:
                continue
            xs, ys = x[a:b].float(), cand[c:d].float()
            dm = ((xs * xs).sum(1)[:, None] + (ys * ys).sum(1)[None, :] - 2.0 * (xs @ ys.t())).clamp_min(0)
            order = torch.sort(dm, dim=1, stable=True).indices   # ties: the lower j
            if excl:
                rows = torch.arange(b - a, device=x.device)[:, None]
                order = order[order != rows].view(b - a, d - c - 1)
            order = order[:, :keep]
            ids.append((order + c).reshape(-1))
            ds.append(torch.gather(dm, 1, order).reshape(-1))
        idx = torch.cat(ids).to(torch.int32) if ids else torch.empty(0, dtype=torch.int32, device=x.device)
        dist = (torch.cat(ds) if ds else torch.empty(0, dtype=torch.float32, device=x.device)) if return_dist else None
    blk = Block(out_ptr, idx, None, None, n, m, num_e)
    return (blk, dist) if return_dist else blk
