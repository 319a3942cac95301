"""CPU: gnnagg_block_rgcn_run (include/gnnagg.h section F, "Block R-GCN layer") without a device -- every refusal of the C-ABI and of
Block.rgcn, each naming its argument and decided before any device work, and gnnagg_block_rgcn_supported at the edges of its rule."""
import re

import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

NAME = "gnnagg_block_rgcn_run"
F32, B16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
# a call that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD = dict(ptr=0x1000, idx=0x2000, num_dst=4, src=0x3000, etype=0x3800, etype_eid=0x5000, val=0x4000, val_eid=0x5000, x=0x6000, x_dtype=B16,
            x_pitch=16, feat=16, w_self=0x7000, w_rel=0x8000, num_rel=3, bias=0x9000, n_out=8, out=0xa000, out_dtype=B16,
            reduce=_lib.REDUCE_MEAN, flags=_lib.FLAG_RELU, stream=None)

REFUSALS = [
    ("negative num_dst", dict(num_dst=-1), "num_dst"),
    ("feat 0", dict(feat=0), "feat"),
    ("n_out 0", dict(n_out=0), "n_out"),
    ("num_rel 0", dict(num_rel=0), "num_rel"),
    ("pitch below feat", dict(x_pitch=15), "x_pitch"),
    ("unknown x dtype", dict(x_dtype=2), "x_dtype"),
    ("unknown out dtype", dict(out_dtype=-1), "out_dtype"),
    ("fp32 operands, bf16 out", dict(x_dtype=F32), "out_dtype"),
    ("there is no max", dict(reduce=_lib.REDUCE_MAX), "reduce"),
    ("the accumulate flag", dict(flags=_lib.FLAG_ACCUMULATE), "flags"),
    ("val_eid without val", dict(val=None), "d_val_eid"),
    ("etype_eid without etype", dict(etype=None), "d_etype_eid"),
    ("feat past the range", dict(feat=257, x_pitch=257), "feat"),
    ("n_out past the range", dict(n_out=257), "n_out"),
    ("relations past the LDS", dict(feat=128, x_pitch=128, n_out=64, num_rel=8), "gnnagg_block_rgcn_supported"),
    ("null blk_ptr", dict(ptr=None), "d_blk_ptr"),
    ("null etype", dict(etype=None, etype_eid=None), "d_etype"),
    ("null x", dict(x=None), "d_x"),
    ("null w_rel", dict(w_rel=None), "d_w_rel"),
    ("null out", dict(out=None), "d_out"),
]


def call(**over):
    return gnc.lib().gnnagg_block_rgcn_run(*dict(GOOD, **over).values())


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, over, word):
    assert call(**over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_num_dst_0_launches_nothing_and_still_refuses_what_is_wrong():
    nothing = dict.fromkeys(("ptr", "idx", "src", "etype", "etype_eid", "val", "val_eid", "x", "w_self", "w_rel", "bias", "out"))
    assert call(num_dst=0, **nothing) == _lib.OK
    assert call(num_dst=0, num_rel=0) == _lib.ERR_ARG


# the rule: feat, n_out <= 256, num_rel >= 1 and 64 + roundup16(64 R) + tile (+ bf16: 64 R roundup4(feat) + the image) <= 160 KB.
# fp32 256 columns: 16 rows x (256 (R + 1) + 4) x 4 bytes -- R = 8 is 147 KB, R = 9 is 164 KB.  bf16 128 -> 64: R = 4 is 20 KB of
# tile + 32 KB of running sums + 81 KB of image, R = 5 is 161.5 KB with its counts.
SUPPORTED = [(1, 1, 1, F32, 1), (256, 256, 8, F32, 1), (256, 256, 9, F32, 0), (128, 64, 18, F32, 1), (128, 64, 19, F32, 0), (257, 1, 1, F32, 0),
             (1, 257, 1, F32, 0), (8, 8, 0, F32, 0), (8, 8, -1, B16, 0), (0, 8, 1, F32, 0), (8, 0, 1, B16, 0), (1, 1, 1 << 30, F32, 0),
             (128, 64, 4, B16, 1), (128, 64, 5, B16, 0), (128, 256, 1, B16, 1), (256, 129, 1, B16, 0), (32, 16, 2, 2, 0)]


@pytest.mark.parametrize("feat,n_out,num_rel,dt,want", SUPPORTED)
def test_supported_at_the_edges_of_its_rule(feat, n_out, num_rel, dt, want):
    L = gnc.lib()
    assert L.gnnagg_block_rgcn_supported(feat, n_out, num_rel, dt) == want
    if not want:
        assert L.gnnagg_block_rgcn_grid_cap(feat, n_out, num_rel, dt) == 0   # (inside the range the cap asks the device for its CUs)
    if dt in (F32, B16):
        assert gnc.block_rgcn_supported(feat, n_out, num_rel, torch.float32 if dt == F32 else torch.bfloat16) == bool(want)


# ------------------------------------------------------------------------------------------------------------ the wrapper
def cpu_block(eid=False):
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return gnc.Block(i32([0, 2, 2]), i32([1, 0]), i32([5, 7]), i32([3, 9]) if eid else None, 2, 2, 2)


X, W, T = torch.zeros(10, 4), torch.zeros(2, 4, 3), torch.zeros(2, dtype=torch.int32)
WRAPPER = [
    ("there is no max", cpu_block(), dict(x=X, w_rel=W, etype=T, reduce="max"), ValueError, "reduce"),
    ("etype_full without eid", cpu_block(), dict(x=X, w_rel=W, etype=T, etype_full=True), ValueError, "eid"),
    ("val_full without val", cpu_block(eid=True), dict(x=X, w_rel=W, etype=T, val_full=True), ValueError, "val"),
    ("out_dtype float16", cpu_block(), dict(x=X, w_rel=W, etype=T, out_dtype=torch.float16), TypeError, "out_dtype"),
    ("x float16", cpu_block(), dict(x=X.half(), w_rel=W.half(), etype=T), TypeError, "x must be"),
    ("a gathered x with too few rows", cpu_block(), dict(x=torch.zeros(1, 4), w_rel=W, etype=T, gathered=True), ValueError, "rows"),
    ("etype int64", cpu_block(), dict(x=X, w_rel=W, etype=T.long()), TypeError, "etype"),
    ("etype of the wrong length", cpu_block(), dict(x=X, w_rel=W, etype=torch.zeros(3, dtype=torch.int32)), ValueError, "etype"),
    ("val of the wrong length", cpu_block(), dict(x=X, w_rel=W, etype=T, val=torch.zeros(3)), ValueError, "val"),
    ("w_rel of another dtype", cpu_block(), dict(x=X, w_rel=W.bfloat16(), etype=T), TypeError, "w_rel"),
    ("w_rel 2-D", cpu_block(), dict(x=X, w_rel=W[0], etype=T), ValueError, "w_rel"),
    ("w_rel with other rows", cpu_block(), dict(x=X, w_rel=torch.zeros(2, 5, 3), etype=T), ValueError, "w_rel"),
    ("w_self of another dtype", cpu_block(), dict(x=X, w_rel=W, etype=T, w_self=W[0].bfloat16()), TypeError, "w_self"),
    ("w_self of another shape", cpu_block(), dict(x=X, w_rel=W, etype=T, w_self=torch.zeros(4, 2)), ValueError, "w_self"),
    ("bias of the wrong length", cpu_block(), dict(x=X, w_rel=W, etype=T, bias=torch.zeros(4)), ValueError, "bias"),
    ("out of the wrong shape", cpu_block(), dict(x=X, w_rel=W, etype=T, out=torch.zeros(2, 4)), ValueError, "out must be"),
    ("a bfloat16 out of float32 operands", cpu_block(), dict(x=X, w_rel=W, etype=T, out_dtype=torch.bfloat16), TypeError, "out_dtype"),
    ("fused=True outside the range", cpu_block(), dict(x=torch.zeros(10, 300), w_rel=torch.zeros(2, 300, 3), etype=T, fused=True), ValueError,
     "fused=True"),
    ("x on the host", cpu_block(), dict(x=X, w_rel=W, etype=T), ValueError, "device tensor"),
    ("x on the host, composition", cpu_block(), dict(x=X, w_rel=W, etype=T, fused=False), ValueError, "device tensor"),   # no CPU arm
]


@pytest.mark.parametrize("what,blk,kw,exc,word", WRAPPER, ids=[w[0] for w in WRAPPER])
def test_wrapper_refusals_are_raised_before_device_work(what, blk, kw, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        blk.rgcn(**kw)
    with pytest.raises(exc, match=re.escape(word)):
        gnc.block_rgcn_run(blk, **kw)
