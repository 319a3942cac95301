"""Host-side mirror of the reference's operator interface, over the C-ABI of libgnnagg.so.

Two surfaces, both taking torch tensors that live in HIP device memory (torch is only the
allocator / stream provider here; all compute happens in the hand-written HIP kernels):

* classes ``Aggregator_GCN`` / ``Aggregator_GAT`` with the method names, argument order and
  semantics of reference include/aggr_gcn.h:362-550 and include/aggr_gat.h:299-441;
* the flat functions the reference's pybind module exports (Figure7/kernel.cpp:166-179):
  ``new_load, gcn_init, gcn_update_val, gcn_run, gcn_schedule, gat_init, gat_run, gat_schedule,
  gat_run_u_add_v, gat_run_add_to_center, gat_run_div_each`` -- a script written against the
  reference extension (Figure7/our.py:79-84,171-188) runs unchanged with
  ``import gnn_computing_amd as gnc``.
"""
import ctypes
import enum
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, lib


class Schedule(enum.IntEnum):
    """reference include/graph_schedule.h:8-14"""
    locality = _lib.SCHED_LOCALITY
    neighbor_grouping = _lib.SCHED_NEIGHBOR_GROUPING
    locality_neighbor_grouping = _lib.SCHED_LOCALITY_NEIGHBOR_GROUPING
    nop = _lib.SCHED_NOP


REDUCE = {"sum": _lib.REDUCE_SUM, "mean": _lib.REDUCE_MEAN, "max": _lib.REDUCE_MAX}
MODE = {"rows": _lib.MODE_ROWS, "scheduled": _lib.MODE_SCHEDULED, "balanced": _lib.MODE_BALANCED}
AGGRS = {"sum": _lib.AGGR_SUM, "mean": _lib.AGGR_MEAN, "min": _lib.AGGR_MIN, "max": _lib.AGGR_MAX, "var": _lib.AGGR_VAR,
         "std": _lib.AGGR_STD}   # gnnagg_gcn_run_multi
SCALERS = {"identity": _lib.SCALER_IDENTITY, "amplification": _lib.SCALER_AMPLIFICATION, "attenuation": _lib.SCALER_ATTENUATION}
FEATURE_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16}   # gnnagg_gcn_run_typed / gnnagg_gat_run_typed


def _feat_dtype(t, name):
    """GNNAGG_DTYPE_* of a feature tensor (GCN / GAT vin, vout); raises TypeError for anything but float32 / bfloat16, before any device work"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype not in FEATURE_DTYPES:
        raise TypeError("%s must be torch.float32 or torch.bfloat16, got %s" % (name, t.dtype))
    return FEATURE_DTYPES[t.dtype]


def _dev_ptr(t, dtype, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise ValueError("%s must be a HIP device tensor (kernel.cpp:71 CHECK_CUDA)" % name)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous (kernel.cpp:72 CHECK_CONTIGUOUS)" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return ctypes.c_void_p(t.data_ptr())


def _dev_ptr_rows(t, dtype, name):
    """_dev_ptr for a row-pitched 2-D view (unit column stride, rows stride(0) elements apart): (pointer, pitch in elements); never a copy"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.dim() != 2:
        raise ValueError("%s must be 2-D [rows, F], got %s" % (name, tuple(t.shape)))
    if t.shape[1] != 1 and t.stride(1) != 1:
        raise ValueError("%s must have stride(1) == 1 (a column view of a row-major tensor), got strides %s" % (name, tuple(t.stride())))
    pitch = int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))
    if pitch < t.shape[1]:
        raise ValueError("%s: row pitch stride(0) = %d is below its %d columns" % (name, pitch, t.shape[1]))
    if not t.is_cuda:
        raise ValueError("%s must be a HIP device tensor (kernel.cpp:71 CHECK_CUDA)" % name)
    return ctypes.c_void_p(t.data_ptr()), pitch


def _need_extras(what):
    """the backward entry points are out of scope and ship in libgnnagg_extras.so only"""
    if not _lib.has_extras():
        raise RuntimeError("%s: the loaded libgnnagg.so has no backward entry points (SURVEY.md 2.2: out of scope); build "
                           "`make -C gnn_computing_amd/csrc extras` and load it with GNNAGG_LIB=.../libgnnagg_extras.so" % what)


def _mode(scheduled):
    if isinstance(scheduled, str):
        return MODE[scheduled]
    return _lib.MODE_SCHEDULED if scheduled else _lib.MODE_ROWS


def _bias_heads(bias, num_e, heads, like, who):
    """bias_heads of the score bias of run_v2 / run_dot: a contiguous float32 [num_e], [num_e, 1] (one value per edge for every head)
    or [num_e, heads] tensor on `like`'s device; raises before any device work"""
    if not isinstance(bias, torch.Tensor):
        raise TypeError("%s: bias must be a torch.Tensor or None" % who)
    if bias.dtype != torch.float32:
        raise TypeError("%s: bias must be torch.float32, got %s" % (who, bias.dtype))
    shape = tuple(bias.shape)
    if shape not in ((num_e,), (num_e, 1), (num_e, heads)):
        raise ValueError("%s: bias must be [num_e = %d], [num_e, 1] or [num_e, heads = %d], got %s" % (who, num_e, heads, shape))
    if not bias.is_contiguous():
        raise ValueError("%s: bias must be contiguous, got strides %s" % (who, tuple(bias.stride())))
    if bias.device != like.device:
        raise ValueError("%s: bias is on %s, the operands on %s" % (who, bias.device, like.device))
    return 1 if bias.dim() == 1 else int(shape[1])


def _edge_rows(edge, num_e, feat, like, who):
    """(pointer, pitch in elements) of the per-edge feature rows of run_v2 / run_dot: a [num_e, F] tensor of `like`'s dtype on its device,
    unit column stride, rows stride(0) >= F elements apart (a column view of a wider tensor is taken as it is); raises before any device
    work"""
    if not isinstance(edge, torch.Tensor):
        raise TypeError("%s: edge must be a torch.Tensor or None" % who)
    if edge.dtype != like.dtype:
        raise TypeError("%s: edge must have the operands' dtype %s, got %s" % (who, like.dtype, edge.dtype))
    if edge.dim() != 2:
        raise ValueError("%s: edge must be [num_e = %d, F = %d], got %s" % (who, num_e, feat, tuple(edge.shape)))
    if tuple(edge.shape) != (num_e, feat):
        raise ValueError("%s: edge must be [num_e = %d, F = %d], got %s" % (who, num_e, feat, tuple(edge.shape)))
    if feat != 1 and edge.stride(1) != 1:
        raise ValueError("%s: edge must have stride(1) == 1 (a column view of a row-major tensor), got strides %s" % (who, tuple(edge.stride())))
    if num_e > 1 and edge.stride(0) < feat:
        raise ValueError("%s: edge: row pitch stride(0) = %d is below F = %d" % (who, edge.stride(0), feat))
    if edge.device != like.device:
        raise ValueError("%s: edge is on %s, the operands on %s" % (who, edge.device, like.device))
    return ctypes.c_void_p(edge.data_ptr()), (int(edge.stride(0)) if num_e > 1 else feat)


def _weights_out(weights, stats, num_v, num_e, heads, like, who):
    """the two outputs of the weights form of run_v2 / run_dot: weights, a contiguous float32 tensor of num_e * heads elements on `like`'s
    device ([num_e, heads], or [num_e] at one head), and stats, contiguous float32 [V, heads, 2] (allocated here when None).  Returns
    stats; (None, None) is the call without weights and returns None; raises before any device work.  (A graph without edges has a weights
    tensor without elements, whose pointer is null: the callers hand the library the stats pointer in its place -- nothing is written there.)"""
    if weights is None:
        if stats is not None:
            raise ValueError("%s: stats without weights -- the row statistics come with the attention weights" % who)
        return None
    for t, name, shapes in ((weights, "weights", ((num_e, heads),) + (((num_e,),) if heads == 1 else ())),
                            (stats, "stats", ((num_v, heads, 2),))):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch.Tensor or None" % (who, name))
        if t.dtype != torch.float32:
            raise TypeError("%s: %s must be torch.float32, got %s" % (who, name, t.dtype))
        if tuple(t.shape) not in shapes:
            raise ValueError("%s: %s must be %s, got %s" % (who, name, " or ".join(str(list(x)) for x in shapes), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous, got strides %s" % (who, name, tuple(t.stride())))
        if t.device != like.device:
            raise ValueError("%s: %s is on %s, the operands on %s" % (who, name, t.device, like.device))
    if stats is None:
        stats = torch.empty((num_v, heads, 2), dtype=torch.float32, device=like.device)
    return stats


class Aggregator:
    """reference include/aggregator.h:25-151.  Holds the device CSR (borrowed tensors are kept
    alive by this object) and the scheduled work lists."""

    def __init__(self, ptr, idx, feat_in=32, feat_out=32):
        self.ptr, self.idx = ptr, idx
        self.num_v = int(ptr.numel()) - 1
        self.num_e = int(idx.numel())
        self.feat_in, self.feat_out = feat_in, feat_out
        self._h = ctypes.c_int64(0)

    # -- lifetime
    def close(self):
        if self._h.value:
            lib().gnnagg_destroy(self._h)
            self._h = ctypes.c_int64(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _use_current_stream(self):
        """work of the following call is enqueued on torch's current stream; host-synchronous reads of the caller's arrays (plan
        construction) are ordered behind it too (gnnagg.h: copy_to_host)"""
        check(lib().gnnagg_set_stream(self._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def set_option(self, name, value):
        """Per-handle knob (gnnagg_set_option): "partitions", "tile_width", "slice_kb", "fast_rows", ..."""
        check(lib().gnnagg_set_option(self._h, name.encode(), int(value)))

    # -- aggregator.h:67-99
    def schedule(self, s, param, total_num_v=None):
        arr = (ctypes.c_int * 2)(*(list(param) + [0])[:2])
        self._use_current_stream()   # (plan construction reads the CSR: ordered behind the stream that may still be writing it)
        check(lib().gnnagg_schedule(self._h, int(s), arr, self.num_v if total_num_v is None else int(total_num_v)))

    def plan_info(self):
        """{plan_s, rows_plan_s, plan_bytes, scratch_bytes} of the library-chosen blocked order (gnnagg_plan_info)."""
        a, b, pb, sb = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_longlong(0), ctypes.c_longlong(0)
        check(lib().gnnagg_plan_info(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(pb), ctypes.byref(sb)))
        return {"plan_s": a.value, "rows_plan_s": b.value, "plan_bytes": pb.value, "scratch_bytes": sb.value}

    def schedule_balanced(self, chunk=0):
        self._use_current_stream()
        check(lib().gnnagg_schedule_balanced(self._h, int(chunk)))

    def balanced_params(self):
        """(chunk, seg_chunks) of the balanced mode's summation order (see gnnagg_balanced_params)."""
        ch, sg = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().gnnagg_balanced_params(self._h, ctypes.byref(ch), ctypes.byref(sg)))
        return ch.value, sg.value

    def rows_blocked_ranges(self):
        """0, or the number of source ranges when `scheduled = 0` runs its canonical chains on the 2-D blocked order
        (gnnagg_rows_blocked_ranges; GCN handles)."""
        n = ctypes.c_int(0)
        check(lib().gnnagg_rows_blocked_ranges(self._h, ctypes.byref(n)))
        return n.value

    def balanced_partitions(self):
        """0, or the number of source partitions when the balanced mode chose the partitioned order (gnnagg_balanced_partitions)."""
        n = ctypes.c_int(0)
        check(lib().gnnagg_balanced_partitions(self._h, ctypes.byref(n), None))
        return n.value

    def balanced_partition_columns(self):
        """Column count the source ranges are cut from (largest neighbor id + 1), 0 when not partitioned."""
        n, t = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().gnnagg_balanced_partitions(self._h, ctypes.byref(n), ctypes.byref(t)))
        return t.value

    def mode_params(self, mode="scheduled"):
        """(chunk, seg_chunks) of any mode's summation order (gnnagg_mode_params)."""
        ch, sg = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().gnnagg_mode_params(self._h, MODE[mode], ctypes.byref(ch), ctypes.byref(sg)))
        return ch.value, sg.value

    @property
    def num_target(self):
        """aggregator.h:126"""
        out = ctypes.c_int(0)
        check(lib().gnnagg_num_target(self._h, _lib.MODE_SCHEDULED, ctypes.byref(out)))
        return out.value

    def get_schedule(self, mode="scheduled", with_val=False):
        """Host copies (numpy) of ptr_s, idx_s, target[, val_s] as the kernels consume them."""
        m = MODE[mode]
        n = ctypes.c_int(0)
        check(lib().gnnagg_num_target(self._h, m, ctypes.byref(n)))
        ptr_s = np.empty(n.value + 1, np.int32)
        tgt = np.empty(n.value, np.int32)
        check(lib().gnnagg_get_schedule(self._h, m, ptr_s.ctypes.data, None, tgt.ctypes.data, None))
        ne = int(ptr_s[-1])
        idx_s = np.empty(ne, np.int32)
        val_s = np.empty(ne, np.float32) if with_val else None
        check(lib().gnnagg_get_schedule(self._h, m, None, idx_s.ctypes.data, None,
                                        val_s.ctypes.data if with_val else None))
        return (ptr_s, idx_s, tgt, val_s) if with_val else (ptr_s, idx_s, tgt)

    def check_csr(self, num_cols=0):
        """(rows with ptr[r] > ptr[r+1], neighbor ids outside [0, num_cols)) -- gnnagg_check_csr."""
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        self._use_current_stream()
        check(lib().gnnagg_check_csr(self._h, int(num_cols), ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # -- aggregator.h:115-122
    def csr2edgelist(self):
        out = torch.empty(2 * self.num_e, dtype=torch.int32, device=self.ptr.device)
        self._use_current_stream()
        check(lib().gnnagg_csr2edgelist(self._h, ctypes.c_void_p(out.data_ptr())))
        return out


class Aggregator_GCN(Aggregator):
    """reference include/aggr_gcn.h:362-550"""

    def __init__(self, ptr, idx, val, feat_in=32, feat_out=32):
        super().__init__(ptr, idx, feat_in, feat_out)
        self.val = val
        check(lib().gnnagg_gcn_create(_dev_ptr(ptr, torch.int32, "ptr"), _dev_ptr(idx, torch.int32, "idx"),
                                      _dev_ptr(val, torch.float32, "val"), self.num_v, self.num_e,
                                      ctypes.byref(self._h)))

    def run(self, vin, vout, BLOCK_SIZE=512, scheduled=0, reduce="sum", accumulate=False, relu=False):
        """aggr_gcn.h:379-410.  BLOCK_SIZE is accepted for signature parity and ignored.
        accumulate=True (balanced mode, sum): vout += A.vin.  relu=True: vout = max(result, 0) in the same kernel
        (the F.relu that follows gcn_run in Figure7/our.py:176)."""
        return self.run_with_feat(vin, vout, BLOCK_SIZE, scheduled, int(vin.shape[1]), reduce, accumulate, relu)

    def run_with_feat(self, vin, vout, BLOCK_SIZE, scheduled, feat, reduce="sum", accumulate=False, relu=False):
        """aggr_gcn.h:411-444.  vin / vout: torch.float32 or torch.bfloat16 (extension, gnnagg_gcn_run_typed): the accumulation
        stays fp32, a bfloat16 vout is one round-to-nearest-even of the fp32 result; float32 / float32 is gnnagg_gcn_run_ex."""
        xt, yt = _feat_dtype(vin, "vin"), _feat_dtype(vout, "vout")
        if vout.numel() < self.num_v * feat:
            raise ValueError("vout must hold num_v * feat floats")
        self.feat_in = feat
        flags = (_lib.FLAG_ACCUMULATE if accumulate else 0) | (_lib.FLAG_RELU if relu else 0)
        self._use_current_stream()
        if xt == _lib.DTYPE_F32 and yt == _lib.DTYPE_F32:
            check(lib().gnnagg_gcn_run_ex(self._h, _dev_ptr(vin, torch.float32, "vin"), _dev_ptr(vout, torch.float32, "vout"),
                                          int(feat), _mode(scheduled), REDUCE[reduce], flags))
        else:
            check(lib().gnnagg_gcn_run_typed(self._h, _dev_ptr(vin, vin.dtype, "vin"), xt, _dev_ptr(vout, vout.dtype, "vout"), yt,
                                             int(feat), _mode(scheduled), REDUCE[reduce], flags))
        return 0.0

    def probe_gather(self, vin, scheduled="balanced"):
        """Measurement aid (gnnagg_gcn_probe_gather): the loads of run(vin, ., ., scheduled) without the FMA chains and
        without any store -- the gather ceiling of that launch."""
        self._use_current_stream()
        check(lib().gnnagg_gcn_probe_gather(self._h, _dev_ptr(vin, torch.float32, "vin"), int(vin.shape[1]), _mode(scheduled)))

    def run_clock(self, vin, vout, BLOCK_SIZE=64, scheduled=0):
        """aggr_gcn.h:462-489.  Returns an int64 tensor [blocks, 3] = (start tick, end tick, CU id) per workgroup of
        the one-item-per-lane-group kernel (ticks of gnnagg_wall_clock_hz())."""
        nb = ctypes.c_int(0)
        mode = _mode(scheduled)
        check(lib().gnnagg_gcn_run_clock(self._h, None, None, int(vin.shape[1]), mode, None, ctypes.byref(nb), None))
        timer = torch.zeros((max(nb.value, 1), 3), dtype=torch.int64, device=vin.device)
        self._use_current_stream()
        check(lib().gnnagg_gcn_run_clock(self._h, _dev_ptr(vin, torch.float32, "vin"), _dev_ptr(vout, torch.float32, "vout"),
                                         int(vin.shape[1]), mode, ctypes.c_void_p(timer.data_ptr()), ctypes.byref(nb), None))
        return timer[:nb.value]

    def runEdgeWise(self, vin, vout, BLOCK_SIZE=512, scheduled=0):
        """aggr_gcn.h:446-460"""
        self._use_current_stream()
        check(lib().gnnagg_gcn_run_edgewise(self._h, _dev_ptr(vin, torch.float32, "vin"),
                                            _dev_ptr(vout, torch.float32, "vout"), int(vin.shape[1])))
        return 0.0

    def run_with_nn(self, vin, vout, weight, transformed, BLOCK_SIZE=128, scheduled=1):
        """aggr_gcn.h:491-499: vout = A.vin, transformed = vout @ weight (weight [feat_in, feat_out])."""
        self._use_current_stream()
        check(lib().gnnagg_gcn_run_with_nn(self._h, _dev_ptr(vin, torch.float32, "vin"), _dev_ptr(vout, torch.float32, "vout"),
                                           _dev_ptr(weight, torch.float32, "weight"),
                                           _dev_ptr(transformed, torch.float32, "transformed"), int(vin.shape[1]),
                                           int(weight.shape[1]), _mode(scheduled)))

    def run_with_nn_typed(self, vin, vout, weight, transformed, scheduled="balanced", reduce="sum", relu=False):
        """gnnagg_gcn_run_with_nn_typed: vout = [relu](A.vin) exactly as run() writes it with the same dtypes, and transformed = vout @ weight
        taken from vout AS STORED.  vin float32 / bfloat16; (vout, weight, transformed) = (float32, float32, float32): the ascending-k fp32
        chain of matmul_NN; (bfloat16, bfloat16, float32 | bfloat16): the bf16 MFMA product of matmul_NN with fp32 accumulation.
        vin [V, F], weight [F, N], vout >= V * F elements, transformed >= V * N.  Dtypes and shapes are checked before the library is reached."""
        xt, yt = _feat_dtype(vin, "vin"), _feat_dtype(vout, "vout")
        wt, tt = _feat_dtype(weight, "weight"), _feat_dtype(transformed, "transformed")
        if wt != yt or (yt == _lib.DTYPE_F32 and tt != _lib.DTYPE_F32):
            raise TypeError("run_with_nn_typed: (vout, weight, transformed) must be (float32, float32, float32) or (bfloat16, bfloat16, "
                            "float32 | bfloat16), got (%s, %s, %s)" % (vout.dtype, weight.dtype, transformed.dtype))
        if vin.dim() != 2 or weight.dim() != 2:
            raise ValueError("run_with_nn_typed: vin must be [V, F] and weight [F, N]")
        feat, n_out = int(vin.shape[1]), int(weight.shape[1])
        if int(vin.shape[0]) < self.num_v or int(weight.shape[0]) != feat or feat < 1 or n_out < 1:
            raise ValueError("run_with_nn_typed: vin [%d, %d] and weight [%d, %d] do not fit num_v = %d rows of F features"
                             % (vin.shape[0], feat, weight.shape[0], n_out, self.num_v))
        if vout.numel() < self.num_v * feat:
            raise ValueError("vout must hold num_v * feat elements")
        if transformed.numel() < self.num_v * n_out:
            raise ValueError("transformed must hold num_v * feat_out elements")
        if reduce not in REDUCE:
            raise ValueError("reduce must be one of %s" % sorted(REDUCE))
        self._use_current_stream()
        check(lib().gnnagg_gcn_run_with_nn_typed(self._h, _dev_ptr(vin, vin.dtype, "vin"), xt, _dev_ptr(vout, vout.dtype, "vout"), yt,
                                                 _dev_ptr(weight, weight.dtype, "weight"), wt,
                                                 _dev_ptr(transformed, transformed.dtype, "transformed"), tt, feat, n_out,
                                                 _mode(scheduled), REDUCE[reduce], _lib.FLAG_RELU if relu else 0))

    def run_multi(self, vin, vout, aggrs=("mean", "min", "max", "std"), scalers=("identity",), delta=None):
        """gnnagg_gcn_run_multi (extension; the aggregation stage of PNA / PyG's MultiAggregation): several reductions of the messages
        val * vin[idx] from one gather, times degree scalers.  vin [n_src, F] float32 or bfloat16; vout [V, S * A * F] float32 or bfloat16
        (one rounding of the fp32 value), contiguous, with A = len(aggrs) of "sum", "mean", "min", "max", "var", "std" and S =
        len(scalers) of "identity", "amplification", "attenuation".  Blocks lie scaler-major in the order of the library's bits (the
        order of the names above), whatever order the names are given in: column (s_pos * A + a_pos) * F + c.  delta (pna_delta(ptr): the
        training set's mean of log(d + 1)) is needed by the two non-identity scalers.  Rows without edges are +0.  Everything is checked
        here before the library is reached."""
        xt, yt = _feat_dtype(vin, "vin"), _feat_dtype(vout, "vout")
        aggrs = (aggrs,) if isinstance(aggrs, str) else tuple(aggrs)
        scalers = (scalers,) if isinstance(scalers, str) else tuple(scalers)
        for names, table, what in ((aggrs, AGGRS, "aggrs"), (scalers, SCALERS, "scalers")):
            unknown = [n for n in names if n not in table]
            if unknown or not names or len(set(names)) != len(names):
                raise ValueError("run_multi: %s must be distinct names of %s, got %r" % (what, sorted(table, key=table.get), names))
        amask, smask = sum(AGGRS[n] for n in aggrs), sum(SCALERS[n] for n in scalers)
        if vin.dim() != 2 or vout.dim() != 2:
            raise ValueError("run_multi: vin must be [n_src, F] and vout [V, S * A * F], got %s and %s" % (tuple(vin.shape), tuple(vout.shape)))
        feat = int(vin.shape[1])
        if feat < 1:
            raise ValueError("run_multi: vin has no columns")
        want = (self.num_v, len(scalers) * len(aggrs) * feat)
        if tuple(vout.shape) != want:
            raise ValueError("run_multi: vout must be [V = %d, S * A * F = %d * %d * %d], got %s" % (want[0], len(scalers), len(aggrs), feat, tuple(vout.shape)))
        if smask != _lib.SCALER_IDENTITY:
            if delta is None:
                raise ValueError("run_multi: the amplification and attenuation scalers need delta (pna_delta(ptr))")
            if not (math.isfinite(float(delta)) and float(delta) > 0.0):
                raise ValueError("run_multi: delta = %r must be finite and > 0" % (delta,))
        self._use_current_stream()
        check(lib().gnnagg_gcn_run_multi(self._h, _dev_ptr(vin, vin.dtype, "vin"), xt, _dev_ptr(vout, vout.dtype, "vout"), yt, feat, amask,
                                         smask, ctypes.c_float(1.0 if delta is None else float(delta))))

    def last_nn_path(self):
        """gnnagg_last_nn_path: 0 no run_with_nn / run_with_nn_typed call on this aggregator yet, 1 the product ran as the epilogue of the
        aggregation kernel, 2 as a separate GEMM behind the aggregation."""
        p = ctypes.c_int(0)
        check(lib().gnnagg_last_nn_path(self._h, ctypes.byref(p)))
        return p.value

    def run_bwd(self, doutput, dinput):
        """d(input) = A^T . d(output) for the sum aggregation with this aggregator's edge values (extension: the reference
        is forward-only).  Deterministic gather over the transposed CSR."""
        _need_extras("Aggregator_GCN.run_bwd")
        self._use_current_stream()
        check(lib().gnnagg_gcn_run_bwd(self._h, _dev_ptr(doutput, torch.float32, "doutput"),
                                       _dev_ptr(dinput, torch.float32, "dinput"), int(doutput.shape[1])))

    def set_row_aux(self, row_aux):
        """gnnagg_set_row_aux: per-row degrees (int32 device tensor, or None) for means / maxima computed in two passes over
        disjoint edge sets -- the divisor of reduce="mean", the edges already folded into y for reduce="max" + accumulate."""
        self._row_aux = row_aux
        check(lib().gnnagg_set_row_aux(self._h, _dev_ptr(row_aux, torch.int32, "row_aux")))

    def updateval(self, val):
        """aggr_gcn.h:540-544"""
        self.val = val
        check(lib().gnnagg_update_val(self._h, _dev_ptr(val, torch.float32, "val")))


class Aggregator_GAT(Aggregator):
    """reference include/aggr_gat.h:299-441"""

    # k_gat_row_shift as built (csrc/common.h: kShiftGroup, kShiftHeads, kShiftHubEdges): lanes per short row, heads per pass, and the
    # row length above which the whole workgroup walks a row
    ROW_SHIFT_THRESHOLDS = (8, 4, 1024)

    def __init__(self, ptr, idx, feat_in=32, feat_out=32):
        super().__init__(ptr, idx, feat_in, feat_out)
        check(lib().gnnagg_gat_create(_dev_ptr(ptr, torch.int32, "ptr"), _dev_ptr(idx, torch.int32, "idx"),
                                      self.num_v, self.num_e, ctypes.byref(self._h)))

    def run(self, vin, vatt, vout, BLOCK_SIZE=128, scheduled=0, heads=1, slope=0.2, newval=None, stable=False, shift=None):
        """aggr_gat.h:317-354 (slope 0.2 at :347); heads > 1 takes att [V,H,2].  stable / shift: see run_with_feat."""
        return self.run_with_feat(vin, vatt, vout, BLOCK_SIZE, scheduled, int(vin.shape[1]), heads, slope, newval, stable, shift)

    def row_shift(self, vatt, heads=1, slope=0.2, out=None):
        """gnnagg_gat_row_shift (extension): float32 [V, heads], the maximum over each row's edges of the fp32 leaky logit
        max(s, s * slope), s = att[r, h, 0] + att[src, h, 1]; +0 for rows without edges.  What run(..., stable=True) subtracts."""
        if not isinstance(vatt, torch.Tensor) or vatt.dtype != torch.float32:
            raise TypeError("vatt must be a torch.float32 tensor")
        if vatt.numel() < self.num_v * heads * 2:
            raise ValueError("att must hold at least V*heads*2 floats")
        if out is None:
            out = torch.empty((self.num_v, int(heads)), dtype=torch.float32, device=vatt.device)
        elif out.numel() < self.num_v * heads:
            raise ValueError("out must hold at least V*heads floats")
        self._use_current_stream()
        check(lib().gnnagg_gat_row_shift(self._h, _dev_ptr(vatt, torch.float32, "vatt"), int(heads), ctypes.c_float(slope),
                                         _dev_ptr(out, torch.float32, "out")))
        return out

    def run_with_feat(self, vin, vatt, vout, BLOCK_SIZE, scheduled, feat, heads=1, slope=0.2, newval=None, stable=False, shift=None):
        """aggr_gat.h:355-394.  vin / vout: torch.float32 or torch.bfloat16 (extension, gnnagg_gat_run_typed): weights, sums and the
        softmax division stay fp32, a bfloat16 vout is one round-to-nearest-even of the fp32 result; vatt and newval stay float32;
        float32 / float32 is gnnagg_gat_run.
        stable=True (extension, gnnagg_gat_run_shifted): the overflow-safe edge softmax, every leaky logit minus its row maximum (which
        the library computes first, row_shift); shift=tensor [V, heads] float32: the caller's shift instead.  Neither goes with newval."""
        xt, yt = _feat_dtype(vin, "vin"), _feat_dtype(vout, "vout")
        for t, name in ((vatt, "vatt"), (newval, "newval"), (shift, "shift")):
            if isinstance(t, torch.Tensor) and t.dtype != torch.float32:
                raise TypeError("%s must be torch.float32, got %s" % (name, t.dtype))
        if vatt.numel() < self.num_v * heads * 2:
            raise ValueError("att must hold at least V*heads*2 floats")
        if stable or shift is not None:
            if newval is not None:
                raise _lib.GnnAggError(_lib.ERR_ARG, "Aggregator_GAT.run: stable / shift with newval -- gnnagg_gat_run_shifted has no "
                                                     "newval output (the un-normalised weights of a shifted run are in another scale)")
            if shift is not None and shift.numel() < self.num_v * heads:
                raise ValueError("shift must hold at least V*heads floats")
            self._use_current_stream()
            check(lib().gnnagg_gat_run_shifted(self._h, _dev_ptr(vin, vin.dtype, "vin"), xt, _dev_ptr(vatt, torch.float32, "vatt"),
                                               _dev_ptr(shift, torch.float32, "shift"), _dev_ptr(vout, vout.dtype, "vout"), yt, int(feat),
                                               int(heads), ctypes.c_float(slope), _mode(scheduled)))
            return 0.0
        self._use_current_stream()
        if xt == _lib.DTYPE_F32 and yt == _lib.DTYPE_F32:
            check(lib().gnnagg_gat_run(self._h, _dev_ptr(vin, torch.float32, "vin"), _dev_ptr(vatt, torch.float32, "vatt"),
                                       _dev_ptr(vout, torch.float32, "vout"), int(feat), int(heads),
                                       ctypes.c_float(slope), _mode(scheduled), _dev_ptr(newval, torch.float32, "newval")))
        else:
            check(lib().gnnagg_gat_run_typed(self._h, _dev_ptr(vin, vin.dtype, "vin"), xt, _dev_ptr(vatt, torch.float32, "vatt"),
                                             _dev_ptr(vout, vout.dtype, "vout"), yt, int(feat), int(heads),
                                             ctypes.c_float(slope), _mode(scheduled), _dev_ptr(newval, torch.float32, "newval")))
        return 0.0

    # k_gatv2 as built (csrc/common.h: kGatv2Batch, the id windows of the 8- to 64-lane groups, kGatv2LongEdges, kGatv2SegEdges): the row
    # lengths at which the walk of a row changes -- edges per batch, ids per window, the longest row one lane group walks, the edges of a
    # segment (above it: several workgroups and the ordered merge)
    GATV2_THRESHOLDS = (4, 8, 16, 32, 64, 128, 512)
    GATV2_MAX_FEAT = 1024

    def run_v2(self, xs, xd, a, vout, heads=1, slope=0.2, bias=None, weights=None, stats=None, edge=None):
        """gnnagg_gatv2_run (extension): GATv2 attention, e_ij = a[h] . leaky(xd[i] + xs[j]) per head, max-shifted edge softmax over each row's
        edges and the weighted sum of the xs rows, in one call.  xs [n_src, F], xd [>= V, F]: both float32 or both bfloat16 (xd may be xs);
        a: float32, heads * D elements ([heads, D]); vout [>= V, F] float32 or bfloat16 (one rounding of the fp32 result).  Rows without edges
        are +0.  bias (gnnagg_gatv2_run_bias): float32 [num_e], [num_e, 1] or [num_e, heads], contiguous, added to the score of the edge at
        that position of the CSR (and head) before the softmax; -inf masks the edge.  None is the call without a bias.
        weights (gnnagg_gatv2_run_weights): a contiguous float32 [num_e, heads] tensor ([num_e] at one head) the call fills with the attention
        weight of every (edge position, head); stats: contiguous float32 [V, heads, 2], filled with every (row, head)'s (score maximum, softmax
        denominator) -- allocated here when weights is given and stats is None, and returned; give both to keep a captured call free of
        allocations.  stats without weights is a ValueError; neither is the call without them.
        edge (gnnagg_gatv2_run_edge): a feature row per edge, [num_e, F] of xs's dtype on its device, stride(1) == 1 and stride(0) >= F (a
        column view serves), indexed by the edge's position in the CSR: the score becomes a[h] . leaky(xd[i] + (xs[j] + edge[p])); the summed
        row stays xs[j].  None is the call without it, through the entry points above.  Everything is checked here before the library
        is reached."""
        xt, yt = _feat_dtype(xs, "xs"), _feat_dtype(vout, "vout")
        if _feat_dtype(xd, "xd") != xt:
            raise TypeError("xd (%s) must have xs's dtype %s" % (xd.dtype, xs.dtype))
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float32:
            raise TypeError("a must be a torch.float32 tensor")
        heads = int(heads)
        if xs.dim() != 2:
            raise ValueError("xs must be [n_src, F], got %s" % (tuple(xs.shape),))
        feat = int(xs.shape[1])
        if heads < 1 or feat < 1 or feat % heads != 0:
            raise ValueError("run_v2: heads = %d does not divide F = %d" % (heads, feat))
        if a.numel() != feat:
            raise ValueError("run_v2: a %s does not hold [heads = %d, D = %d]" % (tuple(a.shape), heads, feat // heads))
        if xd.numel() < self.num_v * feat:
            raise ValueError("xd must hold at least V*F elements")
        if vout.numel() < self.num_v * feat:
            raise ValueError("vout must hold at least V*F elements")
        bias_heads = None if bias is None else _bias_heads(bias, self.num_e, heads, xs, "run_v2")
        stats = _weights_out(weights, stats, self.num_v, self.num_e, heads, xs, "run_v2")
        ef = None if edge is None else _edge_rows(edge, self.num_e, feat, xs, "run_v2")
        self._use_current_stream()
        if ef is not None:
            check(lib().gnnagg_gatv2_run_edge(self._h, _dev_ptr(xs, xs.dtype, "xs"), _dev_ptr(xd, xd.dtype, "xd"), xt,
                                              _dev_ptr(a, torch.float32, "a"), ef[0], ef[1], _dev_ptr(vout, vout.dtype, "vout"), yt, feat, heads,
                                              ctypes.c_float(slope), _dev_ptr(bias, torch.float32, "bias"), bias_heads or 1,
                                              None if weights is None else _dev_ptr(weights if self.num_e else stats, torch.float32, "weights"),
                                              _dev_ptr(stats, torch.float32, "stats")))
            return stats
        if weights is not None:
            check(lib().gnnagg_gatv2_run_weights(self._h, _dev_ptr(xs, xs.dtype, "xs"), _dev_ptr(xd, xd.dtype, "xd"), xt,
                                                 _dev_ptr(a, torch.float32, "a"), _dev_ptr(vout, vout.dtype, "vout"), yt, feat, heads,
                                                 ctypes.c_float(slope), _dev_ptr(bias, torch.float32, "bias"), bias_heads or 1,
                                                 _dev_ptr(weights if self.num_e else stats, torch.float32, "weights"),
                                                 _dev_ptr(stats, torch.float32, "stats")))
            return stats
        if bias is None:
            check(lib().gnnagg_gatv2_run(self._h, _dev_ptr(xs, xs.dtype, "xs"), _dev_ptr(xd, xd.dtype, "xd"), xt, _dev_ptr(a, torch.float32, "a"),
                                         _dev_ptr(vout, vout.dtype, "vout"), yt, feat, heads, ctypes.c_float(slope)))
        else:
            check(lib().gnnagg_gatv2_run_bias(self._h, _dev_ptr(xs, xs.dtype, "xs"), _dev_ptr(xd, xd.dtype, "xd"), xt,
                                              _dev_ptr(a, torch.float32, "a"), _dev_ptr(vout, vout.dtype, "vout"), yt, feat, heads,
                                              ctypes.c_float(slope), _dev_ptr(bias, torch.float32, "bias"), bias_heads))

    def run_dot(self, q, k, v, vout, heads=1, scale=None, bias=None, weights=None, stats=None, edge=None):
        """gnnagg_dot_attn_run (extension): scaled dot-product attention over the edges, e_ij = scale * q[i] . k[j] per head (D = F / heads
        columns), max-shifted edge softmax over each row's edges and the weighted sum of the v rows, in one call.  q [>= V, F], k and v
        [n_src, F]: all float32 or all bfloat16, row-pitched views allowed (stride(1) == 1; k and v share stride(0)) -- the column views
        of one [n, 3F] projection are taken as they are, never copied; q, k and v may be one tensor.  vout [>= V, F] float32 or bfloat16
        (one rounding of the fp32 result), contiguous.  scale=None is 1 / sqrt(D).  Rows without edges are +0.  bias
        (gnnagg_dot_attn_run_bias): as run_v2's -- float32 [num_e], [num_e, 1] or [num_e, heads], added to the score; -inf masks the edge;
        None is the call without a bias.  weights / stats (gnnagg_dot_attn_run_weights): as run_v2's -- float32 [num_e, heads] filled with
        the attention weights and float32 [V, heads, 2] with every (row, head)'s (maximum, denominator), which is returned.
        edge (gnnagg_dot_attn_run_edge): as run_v2's -- [num_e, F] of q's dtype, row-pitched views allowed, indexed by the edge's position
        in the CSR: the edge scores k[j] + edge[p] and sums v[j] + edge[p].  None is the call without it.  Everything is
        checked here before the library is reached."""
        xt, yt = _feat_dtype(q, "q"), _feat_dtype(vout, "vout")
        if _feat_dtype(k, "k") != xt or _feat_dtype(v, "v") != xt:
            raise TypeError("k (%s) and v (%s) must have q's dtype %s" % (k.dtype, v.dtype, q.dtype))
        heads = int(heads)
        for t, name in ((q, "q"), (k, "k"), (v, "v")):
            if t.dim() != 2:
                raise ValueError("%s must be [rows, F], got %s" % (name, tuple(t.shape)))
        feat = int(q.shape[1])
        if heads < 1 or feat < 1 or feat % heads != 0:
            raise ValueError("run_dot: heads = %d does not divide F = %d" % (heads, feat))
        if tuple(k.shape) != tuple(v.shape):
            raise ValueError("run_dot: k %s and v %s must have one shape" % (tuple(k.shape), tuple(v.shape)))
        if int(k.shape[1]) != feat:
            raise ValueError("run_dot: k and v have %d columns, q has %d" % (k.shape[1], feat))
        if q.shape[0] < self.num_v:
            raise ValueError("q must hold at least V = %d rows" % self.num_v)
        if vout.numel() < self.num_v * feat:
            raise ValueError("vout must hold at least V*F elements")
        scale = 1.0 / math.sqrt(feat // heads) if scale is None else float(scale)
        if not math.isfinite(scale) or not math.isfinite(ctypes.c_float(scale).value):
            raise ValueError("run_dot: scale = %r is not finite (in fp32)" % (scale,))
        for t, name in ((q, "q"), (k, "k"), (v, "v")):
            if t.shape[1] != 1 and t.stride(1) != 1:
                raise ValueError("%s must have stride(1) == 1 (a column view of a row-major tensor), got strides %s" % (name, tuple(t.stride())))
        if k.shape[0] > 1 and k.stride(0) != v.stride(0):
            raise ValueError("run_dot: k and v must share one row pitch, got stride(0) = %d and %d" % (k.stride(0), v.stride(0)))
        for t, name in ((q, "q"), (k, "k")):
            if t.shape[0] > 1 and t.stride(0) < feat:
                raise ValueError("%s: row pitch stride(0) = %d is below F = %d" % (name, t.stride(0), feat))
        bias_heads = None if bias is None else _bias_heads(bias, self.num_e, heads, q, "run_dot")
        stats = _weights_out(weights, stats, self.num_v, self.num_e, heads, q, "run_dot")
        ef = None if edge is None else _edge_rows(edge, self.num_e, feat, q, "run_dot")
        self._use_current_stream()
        (pq, q_pitch), (pk, kv_pitch), (pv, _) = _dev_ptr_rows(q, q.dtype, "q"), _dev_ptr_rows(k, k.dtype, "k"), _dev_ptr_rows(v, v.dtype, "v")
        py = _dev_ptr(vout, vout.dtype, "vout")
        if ef is not None:
            check(lib().gnnagg_dot_attn_run_edge(self._h, pq, q_pitch, pk, pv, kv_pitch, ef[0], ef[1], xt, py, yt, feat, heads,
                                                 ctypes.c_float(scale), _dev_ptr(bias, torch.float32, "bias"), bias_heads or 1,
                                                 None if weights is None else _dev_ptr(weights if self.num_e else stats, torch.float32, "weights"),
                                                 _dev_ptr(stats, torch.float32, "stats")))
            return stats
        if weights is not None:
            check(lib().gnnagg_dot_attn_run_weights(self._h, pq, q_pitch, pk, pv, kv_pitch, xt, py, yt, feat, heads, ctypes.c_float(scale),
                                                    _dev_ptr(bias, torch.float32, "bias"), bias_heads or 1,
                                                    _dev_ptr(weights if self.num_e else stats, torch.float32, "weights"),
                                                    _dev_ptr(stats, torch.float32, "stats")))
            return stats
        if bias is None:
            check(lib().gnnagg_dot_attn_run(self._h, pq, q_pitch, pk, pv, kv_pitch, xt, py, yt, feat, heads, ctypes.c_float(scale)))
        else:
            check(lib().gnnagg_dot_attn_run_bias(self._h, pq, q_pitch, pk, pv, kv_pitch, xt, py, yt, feat, heads, ctypes.c_float(scale),
                                                 _dev_ptr(bias, torch.float32, "bias"), bias_heads))

    def run_part(self, vin, vatt, vout, den_io, part, heads=1, slope=0.2):
        """gnnagg_gat_run_part: the fused aggregation in two passes over disjoint edge sets of the same rows.  part=1: vout
        receives the numerators, den_io [V, heads] the denominators; part=2: both are added to and the rows divided."""
        self._use_current_stream()
        check(lib().gnnagg_gat_run_part(self._h, _dev_ptr(vin, torch.float32, "vin"), _dev_ptr(vatt, torch.float32, "vatt"),
                                        _dev_ptr(vout, torch.float32, "vout"), int(vin.shape[1]), int(heads), ctypes.c_float(slope),
                                        int(part), _dev_ptr(den_io, torch.float32, "den_io")))

    def probe_gather(self, vin, vatt, scheduled="balanced", heads=1):
        """Measurement aid (gnnagg_gat_probe_gather): the loads of run(vin, vatt, ., ., scheduled, heads) on the 2-D blocked
        order without exp, chains or stores -- the gather ceiling of that launch."""
        self._use_current_stream()
        check(lib().gnnagg_gat_probe_gather(self._h, _dev_ptr(vin, torch.float32, "vin"), _dev_ptr(vatt, torch.float32, "vatt"),
                                            int(vin.shape[1]), int(heads), _mode(scheduled)))

    def run_att(self, in_att, out_val, BLOCK_SIZE=128, heads=1, slope=0.2):
        """aggr_gat.h:395-401"""
        self._use_current_stream()
        check(lib().gnnagg_gat_run_att(self._h, _dev_ptr(in_att, torch.float32, "in_att"),
                                       _dev_ptr(out_val, torch.float32, "out_val"), int(heads), ctypes.c_float(slope)))

    def run_u_add_v(self, in_att, out_val, BLOCK_SIZE=128):
        """aggr_gat.h:402-409"""
        self._use_current_stream()
        check(lib().gnnagg_gat_run_u_add_v(self._h, _dev_ptr(in_att, torch.float32, "in_att"),
                                           _dev_ptr(out_val, torch.float32, "out_val")))

    def run_add_to_center(self, in_val, out_att, BLOCK_SIZE=128):
        """aggr_gat.h:410-417"""
        self._use_current_stream()
        check(lib().gnnagg_gat_run_add_to_center(self._h, _dev_ptr(in_val, torch.float32, "in_val"),
                                                 _dev_ptr(out_att, torch.float32, "out_att")))

    def run_div_each(self, in_att, in_out_val, BLOCK_SIZE=128):
        """aggr_gat.h:418-425"""
        self._use_current_stream()
        check(lib().gnnagg_gat_run_div_each(self._h, _dev_ptr(in_att, torch.float32, "in_att"),
                                            _dev_ptr(in_out_val, torch.float32, "in_out_val")))

    def run_bwd(self, output, doutput, newval, div, infeat, d_a_b, d_feat, relu_l=0.2, BLOCK_SIZE=128):
        """aggr_gat.h:426-434 (kernel :222-296).  Backward of the single-head fused aggregation from the forward pass's
        un-normalised edge weights `newval` [E] and denominators `div` [V]: d_feat [V,F] (through the aggregation) and
        d_a_b [V,2] (centre / source attention terms) are overwritten.  See gnnagg_gat_run_bwd for what the reference
        kernel leaves out."""
        self._use_current_stream()
        _need_extras("Aggregator_GAT.run_bwd")
        check(lib().gnnagg_gat_run_bwd(self._h, _dev_ptr(output, torch.float32, "output"),
                                       _dev_ptr(doutput, torch.float32, "doutput"), _dev_ptr(newval, torch.float32, "newval"),
                                       _dev_ptr(div, torch.float32, "div"), _dev_ptr(infeat, torch.float32, "infeat"),
                                       _dev_ptr(d_a_b, torch.float32, "d_a_b"), _dev_ptr(d_feat, torch.float32, "d_feat"),
                                       float(relu_l), int(infeat.shape[1])))


# ------------------------------------------------------------------------------------------
# Flat functions with the reference pybind names (Figure7/kernel.cpp:166-179).  Handles are
# Python objects here (the reference returns the raw pointer as int64 and leaks it).
# ------------------------------------------------------------------------------------------
def matmul_NN(A, B, C=None, out_dtype=None):
    """include/dense.h:4-23: row-major C = A @ B on the MFMA kernels of libgnnagg.  Device tensors: A and B both float32 (C float32;
    the ascending-k fp32 chain of gnnagg_matmul_nn) or both bfloat16 (C float32 or bfloat16: fp32 accumulation on the bf16 MFMA, a bf16
    C is one rounding of the fp32 one; gnnagg_matmul_nn_typed).  C defaults to out_dtype if given, else to A.dtype."""
    ta, tb = _feat_dtype(A, "A"), _feat_dtype(B, "B")
    if C is not None:
        tc = _feat_dtype(C, "C")
        if out_dtype is not None and out_dtype != C.dtype:
            raise TypeError("C is %s but out_dtype is %s" % (C.dtype, out_dtype))
    else:
        if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
            raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
        tc = FEATURE_DTYPES[A.dtype if out_dtype is None else out_dtype]
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[0]:
        raise ValueError("matmul_NN: A %s and B %s do not multiply" % (tuple(A.shape), tuple(B.shape)))
    M, K = A.shape
    N = B.shape[1]
    if C is None:
        C = torch.empty((M, N), dtype=A.dtype if out_dtype is None else out_dtype, device=A.device)
    elif tuple(C.shape) != (M, N):
        raise ValueError("matmul_NN: C %s is not [%d, %d]" % (tuple(C.shape), M, N))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if A.is_cuda else None   # (a host tensor is refused by _dev_ptr)
    if (ta, tb, tc) == (_lib.DTYPE_F32,) * 3:
        check(lib().gnnagg_matmul_nn(_dev_ptr(A, torch.float32, "A"), _dev_ptr(B, torch.float32, "B"), _dev_ptr(C, torch.float32, "C"),
                                     int(M), int(N), int(K), stream))
    else:   # (mixed operand types, fp32 operands with a bf16 C: refused by the library, which names the combination)
        check(lib().gnnagg_matmul_nn_typed(_dev_ptr(A, A.dtype, "A"), ta, _dev_ptr(B, B.dtype, "B"), tb, _dev_ptr(C, C.dtype, "C"), tc,
                                           int(M), int(N), int(K), stream))
    return C


_last_project_path = 0


def gat_project(x, W, a_dst, a_src, heads=1, feat=None, att=None, out_dtype=None):
    """gnnagg_gat_project: the front half of a GAT layer in one call.  Returns (feat, att):
        feat [M, N] = x [M, K] @ W [K, N], N = heads * D -- bit for bit what matmul_NN(x, W, out_dtype=...) returns;
        att [M, heads, 2] float32, what Aggregator_GAT.run(feat, att, ..., heads=heads) reads: att[r, h, 0] = sum_c feat[r, h D + c] a_dst[h, c]
        (the centre term), att[r, h, 1] the same with a_src (the source term), taken from feat as stored, fp32 products and sums.
    Device tensors, contiguous: x, W, a_dst, a_src all float32 (feat float32) or all bfloat16 (feat bfloat16, or float32 with
    out_dtype=torch.float32 or a float32 `feat`); a_dst / a_src are [heads, D] (any shape of heads * D elements for heads = 1).  feat / att: optional
    outputs to write into.  Runs on torch's current stream.  last_project_path() tells which way the call took."""
    global _last_project_path
    tx, tw = _feat_dtype(x, "x"), _feat_dtype(W, "W")
    for t, name in ((a_dst, "a_dst"), (a_src, "a_src")):
        if _feat_dtype(t, name) != tw:
            raise TypeError("%s must have W's dtype %s, got %s" % (name, W.dtype, t.dtype))
    if tx != tw:
        raise TypeError("x (%s) and W (%s) must have the same dtype" % (x.dtype, W.dtype))
    if feat is not None:
        tf = _feat_dtype(feat, "feat")
        if out_dtype is not None and out_dtype != feat.dtype:
            raise TypeError("feat is %s but out_dtype is %s" % (feat.dtype, out_dtype))
    else:
        if out_dtype is not None and out_dtype not in FEATURE_DTYPES:
            raise TypeError("out_dtype must be torch.float32 or torch.bfloat16, got %s" % (out_dtype,))
        tf = FEATURE_DTYPES[x.dtype if out_dtype is None else out_dtype]
    if tx == _lib.DTYPE_F32 and tf != _lib.DTYPE_F32:
        raise TypeError("gat_project: float32 operands give a float32 feat (nothing is converted)")
    if att is not None and (not isinstance(att, torch.Tensor) or att.dtype != torch.float32):
        raise TypeError("att must be a torch.float32 tensor")
    heads = int(heads)
    if x.dim() != 2 or W.dim() != 2 or x.shape[1] != W.shape[0]:
        raise ValueError("gat_project: x %s and W %s do not multiply" % (tuple(x.shape), tuple(W.shape)))
    M, K = x.shape
    N = W.shape[1]
    if heads < 1 or N % heads != 0:
        raise ValueError("gat_project: heads = %d does not divide W's %d columns" % (heads, N))
    for t, name in ((a_dst, "a_dst"), (a_src, "a_src")):
        if t.numel() != N or (heads > 1 and tuple(t.shape) != (heads, N // heads)):
            raise ValueError("gat_project: %s %s is not [%d, %d]" % (name, tuple(t.shape), heads, N // heads))
    if feat is None:
        feat = torch.empty((M, N), dtype=x.dtype if out_dtype is None else out_dtype, device=x.device)
    elif tuple(feat.shape) != (M, N):
        raise ValueError("gat_project: feat %s is not [%d, %d]" % (tuple(feat.shape), M, N))
    if att is None:
        att = torch.empty((M, heads, 2), dtype=torch.float32, device=x.device)
    elif att.numel() != M * heads * 2:
        raise ValueError("gat_project: att %s does not hold [%d, %d, 2]" % (tuple(att.shape), M, heads))
    for t, name in ((x, "x"), (W, "W"), (a_dst, "a_dst"), (a_src, "a_src"), (feat, "feat"), (att, "att")):
        if not t.is_cuda:
            raise ValueError("%s must be a HIP device tensor" % name)
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    path = ctypes.c_int(0)
    check(lib().gnnagg_gat_project(_dev_ptr(x, x.dtype, "x"), tx, _dev_ptr(W, W.dtype, "W"), tw, _dev_ptr(a_dst, W.dtype, "a_dst"),
                                   _dev_ptr(a_src, W.dtype, "a_src"), _dev_ptr(feat, feat.dtype, "feat"), tf, _dev_ptr(att, torch.float32, "att"),
                                   int(M), int(N), int(K), heads, ctypes.byref(path), stream))
    _last_project_path = path.value
    return feat, att


def last_project_path():
    """Which way the last gat_project call of this process took its attention terms: 0 none yet (or an empty call), 1 the epilogue of the
    GEMM kernel, 2 a row-dot kernel behind the GEMM (gnnagg_gat_project's *path: what the launcher did, not a prediction)."""
    return _last_project_path


def load_graph_host(dset, reorder="", datadir="../data/", shuffle=True):
    """gnnagg_load_graph -> dict of numpy arrays (ptr, idx, rows, reverse_rows)."""
    L = lib()
    nv, ne = ctypes.c_int(0), ctypes.c_int(0)
    P = _lib.P_INT
    pptr, pidx, prow, prrow = P(), P(), P(), P()
    check(L.gnnagg_load_graph(datadir.encode(), dset.encode(), reorder.encode(), int(bool(shuffle)), ctypes.byref(nv),
                              ctypes.byref(ne), ctypes.byref(pptr), ctypes.byref(pidx), ctypes.byref(prow),
                              ctypes.byref(prrow)))
    try:
        V, E = nv.value, ne.value
        out = dict(num_v=V, num_e=E,
                   ptr=np.ctypeslib.as_array(pptr, shape=(V + 1,)).copy(),
                   idx=np.ctypeslib.as_array(pidx, shape=(E,)).copy() if E else np.empty(0, np.int32),
                   rows=None, reverse_rows=None)
        if prow:
            out["rows"] = np.ctypeslib.as_array(prow, shape=(V,)).copy() if V else np.empty(0, np.int32)
            out["reverse_rows"] = np.ctypeslib.as_array(prrow, shape=(V,)).copy() if V else np.empty(0, np.int32)
    finally:
        for p in (pptr, pidx, prow, prrow):
            if p:
                L.gnnagg_free_host(ctypes.cast(p, ctypes.c_void_p))
    return out


def new_load(dset, reorder="", devid=0, datadir="../data/"):
    """kernel.cpp:37-67: returns [ptrs, idxs] as int32 device tensors."""
    g = load_graph_host(dset, reorder, datadir)
    dev = torch.device("cuda", devid)
    return [torch.from_numpy(g["ptr"]).to(dev), torch.from_numpy(g["idx"]).to(dev)]


def gcn_init(ptrs, idxs, val):
    """kernel.cpp:78-95.  Handles made through the reference-named surface start with the reference-facing defaults
    (gnnagg_set_option "reference_defaults"): gcn_run(..., scheduled=0) takes the balanced order -- within 1e-5 of the
    CSR-order chain instead of bit-equal to it; at.set_option("fast_rows", 0) restores the canonical chains."""
    at = Aggregator_GCN(ptrs, idxs, val)
    at.set_option("reference_defaults", 1)
    return at


def gcn_update_val(at, val):
    at.updateval(val)


def gcn_run(at, feat, outfeat, blocksize, scheduled, relu=False):
    """Figure7/kernel.cpp:97-106; relu=True fuses the F.relu that follows it in our.py:176 (extension)."""
    at.run_with_feat(feat, outfeat, blocksize, scheduled, int(feat.shape[1]), relu=relu)


def gcn_run_multi(at, feat, outfeat, aggrs=("mean", "min", "max", "std"), scalers=("identity",), delta=None):
    """Aggregator_GCN.run_multi as a flat function (extension: the reference has one reduction per launch)."""
    return at.run_multi(feat, outfeat, aggrs=aggrs, scalers=scalers, delta=delta)


def pna_delta(ptr):
    """PNA's delta of a graph: the mean over its rows of log(d + 1), d the row's degree (float64 on the host; ptr: the CSR offsets as a
    tensor, array or sequence).  A graph without rows gives 1.0."""
    p = ptr.detach().cpu().numpy() if isinstance(ptr, torch.Tensor) else np.asarray(ptr)
    if p.ndim != 1 or p.size < 1:
        raise ValueError("pna_delta: ptr must be the 1-D CSR offsets [V + 1]")
    d = np.diff(p.astype(np.int64))
    return float(np.log(d.astype(np.float64) + 1.0).mean()) if d.size else 1.0


def gcn_schedule(at, neighbor_num):
    at.schedule(Schedule.neighbor_grouping, [neighbor_num])


def gat_init(ptrs, idxs):
    at = Aggregator_GAT(ptrs, idxs)
    at.set_option("reference_defaults", 1)
    return at


def gat_run(at, feat, att, outfeat, blocksize, scheduled, stable=False):
    """Figure7/kernel.cpp's gat_run; stable=True (extension): the overflow-safe edge softmax (Aggregator_GAT.run_with_feat)."""
    at.run_with_feat(feat, att, outfeat, blocksize, scheduled, int(feat.shape[1]), stable=stable)


def gatv2_run(at, xs, xd, a, out, heads=1, slope=0.2, bias=None, weights=None, stats=None, edge=None):
    """Aggregator_GAT.run_v2 as a flat function (extension: the reference has no GATv2)."""
    return at.run_v2(xs, xd, a, out, heads=heads, slope=slope, bias=bias, weights=weights, stats=stats, edge=edge)


def dot_attn_run(at, q, k, v, out, heads=1, scale=None, bias=None, weights=None, stats=None, edge=None):
    """Aggregator_GAT.run_dot as a flat function (extension: the reference has the unnormalised score only, aggr_sddmm.h)."""
    return at.run_dot(q, k, v, out, heads=heads, scale=scale, bias=bias, weights=weights, stats=stats, edge=edge)


def gat_schedule(at, neighbor_num):
    at.schedule(Schedule.neighbor_grouping, [neighbor_num])


def gat_run_u_add_v(at, att, outval, blocksize):
    at.run_u_add_v(att, outval, blocksize)


def gat_run_add_to_center(at, inval, outatt, blocksize):
    at.run_add_to_center(inval, outatt, blocksize)


def gat_run_div_each(at, inatt, inoutval, blocksize):
    at.run_div_each(inatt, inoutval, blocksize)


# ------------------------------------------------------------------------------------------
# Host graph preparation through the C-ABI (numpy in / numpy out; no GPU needed)
# ------------------------------------------------------------------------------------------
def _np_i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def reorder_csr(ptr, idx, rows):
    """gnnagg_reorder_csr (reference src/data.cu:4-29).  Returns (newptr, newidx, reverse_rows)."""
    ptr, idx, rows = _np_i(ptr), _np_i(idx), _np_i(rows)
    V, E = len(ptr) - 1, len(idx)
    rev = np.empty(V, np.int32)
    rev[rows] = np.arange(V, dtype=np.int32)
    nptr, nidx = np.empty(V + 1, np.int32), np.empty(E, np.int32)
    check(lib().gnnagg_reorder_csr(ptr.ctypes.data, idx.ctypes.data, rows.ctypes.data, rev.ctypes.data, V, E,
                                   nptr.ctypes.data, nidx.ctypes.data))
    return nptr, nidx, rev


def neighbor_grouping_schedule(ptr, ng):
    """gnnagg_neighbor_grouping_schedule (reference graph_schedule.h:91-126) -> (ptr_s, target)."""
    ptr = _np_i(ptr)
    V = len(ptr) - 1
    n = ctypes.c_int(0)
    check(lib().gnnagg_neighbor_grouping_schedule(ptr.ctypes.data, int(ng), V, None, None, ctypes.byref(n)))
    ptr_s, tgt = np.empty(n.value + 1, np.int32), np.empty(n.value, np.int32)
    check(lib().gnnagg_neighbor_grouping_schedule(ptr.ctypes.data, int(ng), V, ptr_s.ctypes.data, tgt.ctypes.data,
                                                  ctypes.byref(n)))
    return ptr_s, tgt


def locality_schedule(ptr, idx, par_num, total_v, ng=0, val=None):
    """gnnagg_locality_schedule (reference graph_schedule.h:17-63 / :156-211)."""
    ptr, idx = _np_i(ptr), _np_i(idx)
    V, E = len(ptr) - 1, len(idx)
    val = None if val is None else np.ascontiguousarray(val, dtype=np.float32)
    ptr_s, idx_s, tgt = np.empty(E + 2, np.int32), np.empty(max(E, 1), np.int32), np.empty(max(E, 1), np.int32)
    val_s = np.empty(max(E, 1), np.float32) if val is not None else None
    n = ctypes.c_int(0)
    check(lib().gnnagg_locality_schedule(ptr.ctypes.data, idx.ctypes.data, None if val is None else val.ctypes.data,
                                         int(par_num), int(ng), V, int(total_v), ptr_s.ctypes.data, idx_s.ctypes.data,
                                         None if val is None else val_s.ctypes.data, tgt.ctypes.data, ctypes.byref(n)))
    G = n.value
    ne = int(ptr_s[G])
    return ptr_s[:G + 1].copy(), idx_s[:ne].copy(), tgt[:G].copy(), (None if val is None else val_s[:ne].copy())


def cluster_reorder(ptr, idx, threshold=0.2, num_perm=64, cluster_cap=64, seed=123, order="first_member", cache_rows=4096):
    """gnnagg_cluster_reorder[_ex] (reference script/cluster2.py).  Returns (rows, num_clusters); rows[i] = old node id
    placed at new position i, ready for graph.write_reorder_file / reorder_csr.  order="first_member" writes the clusters
    as the reference script does; order="cache_greedy" orders them with an LRU model of `cache_rows` feature rows."""
    ptr, idx = _np_i(ptr), _np_i(idx)
    V = len(ptr) - 1
    rows = np.empty(V, np.int32)
    nc = ctypes.c_int(0)
    mode = {"first_member": 0, "cache_greedy": 1}[order]
    check(lib().gnnagg_cluster_reorder_ex(ptr.ctypes.data, idx.ctypes.data, V, ctypes.c_float(threshold), int(num_perm),
                                          int(cluster_cap), ctypes.c_ulonglong(seed), mode, int(cache_rows), rows.ctypes.data,
                                          ctypes.byref(nc)))
    return rows, nc.value


def partition_rows(ptr, nparts):
    ptr = _np_i(ptr)
    b = np.empty(nparts + 1, np.int32)
    check(lib().gnnagg_partition_rows(ptr.ctypes.data, len(ptr) - 1, int(nparts), b.ctypes.data))
    return b


def halo_plan(ptr, idx, bounds, rank, row_slice=False, num_cols=None):
    """gnnagg_halo_plan / gnnagg_halo_plan_slice -> dict(local_ptr, local_idx, halo_ids, halo_counts).  row_slice=True:
    (ptr, idx) hold the rank's own rows only (ptr[0 .. n_local] with any base, global column ids in idx)."""
    ptr, idx, bounds = _np_i(ptr), _np_i(idx), _np_i(bounds)
    nparts = len(bounds) - 1
    r0, r1 = int(bounds[rank]), int(bounds[rank + 1])
    if row_slice:
        if len(ptr) != r1 - r0 + 1:
            raise ValueError("row slice must have bounds[rank+1] - bounds[rank] + 1 ptr entries")
        nnz = int(ptr[-1] - ptr[0])
    else:
        nnz = int(ptr[r1] - ptr[r0])
    lptr, lidx = np.empty(r1 - r0 + 1, np.int32), np.empty(max(nnz, 1), np.int32)
    counts = np.empty(nparts, np.int32)
    ids_p, nh = _lib.P_INT(), ctypes.c_int(0)
    if row_slice:
        check(lib().gnnagg_halo_plan_slice(ptr.ctypes.data, idx.ctypes.data, int(num_cols), bounds.ctypes.data, nparts, int(rank),
                                           lptr.ctypes.data, lidx.ctypes.data, ctypes.byref(ids_p), counts.ctypes.data,
                                           ctypes.byref(nh)))
    else:
        check(lib().gnnagg_halo_plan(ptr.ctypes.data, idx.ctypes.data, len(ptr) - 1, bounds.ctypes.data, nparts, int(rank),
                                     lptr.ctypes.data, lidx.ctypes.data, ctypes.byref(ids_p), counts.ctypes.data,
                                     ctypes.byref(nh)))
    ids = np.ctypeslib.as_array(ids_p, shape=(nh.value,)).copy() if nh.value else np.empty(0, np.int32)
    lib().gnnagg_free_host(ctypes.cast(ids_p, ctypes.c_void_p))
    return dict(local_ptr=lptr, local_idx=lidx[:nnz].copy(), halo_ids=ids, halo_counts=counts, n_local=r1 - r0)
