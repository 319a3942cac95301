"""CPU: gnnagg_block_sage_run (include/gnnagg.h section F, "Block SAGE layer") without a device -- every refusal of the C-ABI and of
Block.sage, each naming its argument and decided before any device work, and gnnagg_block_sage_supported at the edges of its rule."""
import re

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

NAME = "gnnagg_block_sage_run"
F32, B16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
# a call that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD = dict(ptr=0x1000, idx=0x2000, num_dst=4, src=0x3000, val=0x4000, eid=0x5000, x=0x6000, x_dtype=B16, x_pitch=16, feat=16, w_self=0x7000,
            w_neigh=0x8000, bias=0x9000, n_out=8, out=0xa000, out_dtype=B16, reduce=_lib.REDUCE_MEAN, flags=_lib.FLAG_RELU, stream=None)

REFUSALS = [
    ("negative num_dst", dict(num_dst=-1), "num_dst"),
    ("feat 0", dict(feat=0), "feat"),
    ("n_out 0", dict(n_out=0), "n_out"),
    ("pitch below feat", dict(x_pitch=15), "x_pitch"),
    ("unknown x dtype", dict(x_dtype=2), "x_dtype"),
    ("unknown out dtype", dict(out_dtype=-1), "out_dtype"),
    ("fp32 operands, bf16 out", dict(x_dtype=F32), "out_dtype"),
    ("unknown reduce", dict(reduce=3), "reduce"),
    ("the accumulate flag", dict(flags=_lib.FLAG_ACCUMULATE), "flags"),
    ("eid without val", dict(val=None), "d_eid"),
    ("feat past the range", dict(feat=257, x_pitch=257), "feat"),
    ("n_out past the range", dict(n_out=257), "n_out"),
    ("a bf16 image past the LDS", dict(feat=256, x_pitch=256, n_out=144), "gnnagg_block_sage_supported"),
    ("null blk_ptr", dict(ptr=None), "d_blk_ptr"),
    ("null x", dict(x=None), "d_x"),
    ("null w_neigh", dict(w_neigh=None), "d_w_neigh"),
    ("null out", dict(out=None), "d_out"),
]


def call(**over):
    return gnc.lib().gnnagg_block_sage_run(*dict(GOOD, **over).values())


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, over, word):
    assert call(**over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_num_dst_0_launches_nothing_and_still_refuses_what_is_wrong():
    assert call(num_dst=0, ptr=None, idx=None, x=None, w_self=None, w_neigh=None, bias=None, out=None, src=None, val=None, eid=None) == _lib.OK
    assert call(num_dst=0, n_out=0) == _lib.ERR_ARG


SUPPORTED = [(1, 1, F32, 1), (256, 256, F32, 1), (257, 1, F32, 0), (1, 257, F32, 0), (0, 8, F32, 0), (8, 0, B16, 0), (128, 128, B16, 1),
             (128, 256, B16, 1), (256, 128, B16, 1), (256, 129, B16, 0), (129, 256, B16, 0), (128, 128, 2, 0)]


@pytest.mark.parametrize("feat,n_out,dt,want", SUPPORTED)
def test_supported_at_the_edges_of_its_rule(feat, n_out, dt, want):
    L = gnc.lib()
    assert L.gnnagg_block_sage_supported(feat, n_out, dt) == want
    if not want:
        assert L.gnnagg_block_sage_grid_cap(feat, n_out, dt) == 0       # (inside the range the cap asks the device for its CUs)
    if dt in (F32, B16):
        assert gnc.block_sage_supported(feat, n_out, torch.float32 if dt == F32 else torch.bfloat16) == bool(want)


# ------------------------------------------------------------------------------------------------------------ the wrapper
def cpu_block(eid=False, relabel=True):
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return gnc.Block(i32([0, 2, 2]), i32([1, 0]), i32([5, 7]) if relabel else None, i32([3, 9]) if eid else None, 2, 2 if relabel else 10, 2)


X, W = torch.zeros(10, 4), torch.zeros(4, 3)
WRAPPER = [
    ("unknown reduce", cpu_block(), dict(x=X, w_neigh=W, reduce="prod"), ValueError, "reduce"),
    ("val_full without eid", cpu_block(), dict(x=X, w_neigh=W, val=torch.zeros(20), val_full=True), ValueError, "eid"),
    ("val_full without val", cpu_block(eid=True), dict(x=X, w_neigh=W, val_full=True), ValueError, "val"),
    ("out_dtype float16", cpu_block(), dict(x=X, w_neigh=W, out_dtype=torch.float16), TypeError, "out_dtype"),
    ("x float16", cpu_block(), dict(x=X.half(), w_neigh=W.half()), TypeError, "x must be"),
    ("x 1-D", cpu_block(), dict(x=torch.zeros(10), w_neigh=W), ValueError, "2-D"),
    ("a gathered x with too few rows", cpu_block(), dict(x=torch.zeros(1, 4), w_neigh=W, gathered=True), ValueError, "rows"),
    ("val of the wrong length", cpu_block(), dict(x=X, w_neigh=W, val=torch.zeros(3)), ValueError, "val"),
    ("w_neigh no tensor", cpu_block(), dict(x=X, w_neigh=np.zeros((4, 3), np.float32)), TypeError, "w_neigh"),
    ("w_neigh of another dtype", cpu_block(), dict(x=X, w_neigh=W.bfloat16()), TypeError, "w_neigh"),
    ("w_neigh with other rows", cpu_block(), dict(x=X, w_neigh=torch.zeros(5, 3)), ValueError, "w_neigh"),
    ("w_self of another dtype", cpu_block(), dict(x=X, w_neigh=W, w_self=W.bfloat16()), TypeError, "w_self"),
    ("w_self of another shape", cpu_block(), dict(x=X, w_neigh=W, w_self=torch.zeros(4, 2)), ValueError, "w_self"),
    ("bias bfloat16", cpu_block(), dict(x=X, w_neigh=W, bias=torch.zeros(3, dtype=torch.bfloat16)), TypeError, "bias"),
    ("bias of the wrong length", cpu_block(), dict(x=X, w_neigh=W, bias=torch.zeros(4)), ValueError, "bias"),
    ("out of the wrong shape", cpu_block(), dict(x=X, w_neigh=W, out=torch.zeros(2, 4)), ValueError, "out must be"),
    ("out against out_dtype", cpu_block(), dict(x=X.bfloat16(), w_neigh=W.bfloat16(), out=torch.zeros(2, 3), out_dtype=torch.bfloat16), TypeError,
     "out_dtype"),
    ("a bfloat16 out of float32 operands", cpu_block(), dict(x=X, w_neigh=W, out_dtype=torch.bfloat16), TypeError, "out_dtype"),
    ("fused=True outside the range", cpu_block(), dict(x=torch.zeros(10, 300), w_neigh=torch.zeros(300, 3), fused=True), ValueError, "fused=True"),
    ("x on the host", cpu_block(), dict(x=X, w_neigh=W), ValueError, "device tensor"),
    ("x on the host, composition", cpu_block(), dict(x=X, w_neigh=W, fused=False), ValueError, "device tensor"),
]


@pytest.mark.parametrize("what,blk,kw,exc,word", WRAPPER, ids=[w[0] for w in WRAPPER])
def test_wrapper_refusals_are_raised_before_device_work(what, blk, kw, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        blk.sage(**kw)
    with pytest.raises(exc, match=re.escape(word)):
        gnc.block_sage_run(blk, **kw)
