"""CPU: gnnagg_block_gin_run (include/gnnagg.h section F, "Block GIN layer") without a device -- every refusal of the C-ABI and of
Block.gin, each naming its argument and decided before any device work, and gnnagg_block_gin_supported at the edges of its rule."""
import re

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

NAME = "gnnagg_block_gin_run"
F32, B16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
# a call that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD = dict(ptr=0x1000, idx=0x2000, num_dst=4, src=0x3000, val=0x4000, eid=0x5000, x=0x6000, x_dtype=B16, x_pitch=16, feat=16, self_scale=1.25,
            w1=0x7000, b1=0x8000, hidden=24, w2=0x9000, b2=0xa000, n_out=8, out=0xb000, out_dtype=B16, reduce=_lib.REDUCE_SUM,
            flags=_lib.FLAG_RELU, stream=None)

REFUSALS = [
    ("negative num_dst", dict(num_dst=-1), "num_dst"),
    ("feat 0", dict(feat=0), "feat"),
    ("hidden 0", dict(hidden=0), "hidden"),
    ("n_out 0", dict(n_out=0), "n_out"),
    ("pitch below feat", dict(x_pitch=15), "x_pitch"),
    ("unknown x dtype", dict(x_dtype=2), "x_dtype"),
    ("unknown out dtype", dict(out_dtype=-1), "out_dtype"),
    ("fp32 operands, bf16 out", dict(x_dtype=F32), "out_dtype"),
    ("unknown reduce", dict(reduce=3), "reduce"),
    ("the accumulate flag", dict(flags=_lib.FLAG_ACCUMULATE), "flags"),
    ("an infinite self_scale", dict(self_scale=float("inf")), "self_scale"),
    ("a NaN self_scale", dict(self_scale=float("nan")), "self_scale"),
    ("eid without val", dict(val=None), "d_eid"),
    ("feat past the range", dict(feat=257, x_pitch=257), "feat"),
    ("hidden past the range", dict(hidden=257), "hidden"),
    ("n_out past the range", dict(n_out=257), "n_out"),
    ("bf16 images past the LDS", dict(feat=256, x_pitch=256, hidden=256, n_out=64), "gnnagg_block_gin_supported"),
    ("null blk_ptr", dict(ptr=None), "d_blk_ptr"),
    ("null x", dict(x=None), "d_x"),
    ("null w1", dict(w1=None), "d_w1"),
    ("null w2", dict(w2=None), "d_w2"),
    ("null out", dict(out=None), "d_out"),
]


def call(**over):
    return gnc.lib().gnnagg_block_gin_run(*dict(GOOD, **over).values())


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, over, word):
    assert call(**over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_num_dst_0_launches_nothing_and_still_refuses_what_is_wrong():
    assert call(num_dst=0, ptr=None, idx=None, x=None, w1=None, b1=None, w2=None, b2=None, out=None, src=None, val=None, eid=None) == _lib.OK
    assert call(num_dst=0, hidden=0) == _lib.ERR_ARG


# bf16: 128 + 32 (Fp + 8) + 32 (Hp + 8) + 2 roundup16(hidden) (Fp + 8) + 2 roundup16(n_out) (Hp + 8) bytes against 163 840, Fp / Hp = feat /
# hidden rounded up to 32: 128 -> 128 -> 128 is 78 464, 256 -> 128 -> 64 is 97 920, 256 -> 256 -> 16 is 160 640 and -> 17 (32 image rows)
# 169 088, 128 -> 256 -> 144 is 158 592 and -> 145 (160 image rows) 167 040, 256 -> 256 -> 64 is 185 984.  fp32 256 -> 256 -> 256: 33 408.
SUPPORTED = [(1, 1, 1, F32, 1), (256, 256, 256, F32, 1), (257, 1, 1, F32, 0), (1, 257, 1, F32, 0), (1, 1, 257, F32, 0), (0, 8, 8, F32, 0),
             (8, 0, 8, B16, 0), (8, 8, 0, B16, 0), (128, 128, 128, B16, 1), (256, 128, 64, B16, 1), (256, 256, 64, B16, 0), (256, 256, 16, B16, 1),
             (256, 256, 17, B16, 0), (128, 256, 144, B16, 1), (128, 256, 145, B16, 0), (128, 128, 128, 2, 0)]


@pytest.mark.parametrize("feat,hidden,n_out,dt,want", SUPPORTED)
def test_supported_at_the_edges_of_its_rule(feat, hidden, n_out, dt, want):
    L = gnc.lib()
    assert L.gnnagg_block_gin_supported(feat, hidden, n_out, dt) == want
    if not want:
        assert L.gnnagg_block_gin_grid_cap(feat, hidden, n_out, dt) == 0       # (inside the range the cap asks the device for its CUs)
    if dt in (F32, B16):
        assert gnc.block_gin_supported(feat, hidden, n_out, torch.float32 if dt == F32 else torch.bfloat16) == bool(want)


# ------------------------------------------------------------------------------------------------------------ the wrapper
def cpu_block(eid=False, relabel=True):
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return gnc.Block(i32([0, 2, 2]), i32([1, 0]), i32([5, 7]) if relabel else None, i32([3, 9]) if eid else None, 2, 2 if relabel else 10, 2)


X, W1, W2 = torch.zeros(10, 4), torch.zeros(4, 5), torch.zeros(5, 3)
OK = dict(x=X, w1=W1, w2=W2)
WRAPPER = [
    ("unknown reduce", cpu_block(), dict(OK, reduce="prod"), ValueError, "reduce"),
    ("val_full without eid", cpu_block(), dict(OK, val=torch.zeros(20), val_full=True), ValueError, "eid"),
    ("val_full without val", cpu_block(eid=True), dict(OK, val_full=True), ValueError, "val"),
    ("out_dtype float16", cpu_block(), dict(OK, out_dtype=torch.float16), TypeError, "out_dtype"),
    ("an eps that overflows", cpu_block(), dict(OK, eps=1e39), ValueError, "eps"),
    ("x float16", cpu_block(), dict(x=X.half(), w1=W1.half(), w2=W2.half()), TypeError, "x must be"),
    ("x 1-D", cpu_block(), dict(OK, x=torch.zeros(10)), ValueError, "2-D"),
    ("a gathered x with too few rows", cpu_block(), dict(OK, x=torch.zeros(1, 4), gathered=True), ValueError, "rows"),
    ("val of the wrong length", cpu_block(), dict(OK, val=torch.zeros(3)), ValueError, "val"),
    ("w1 no tensor", cpu_block(), dict(OK, w1=np.zeros((4, 5), np.float32)), TypeError, "w1"),
    ("w2 of another dtype", cpu_block(), dict(OK, w2=W2.bfloat16()), TypeError, "w2"),
    ("w1 with other rows", cpu_block(), dict(OK, w1=torch.zeros(5, 5)), ValueError, "w1"),
    ("w2 that does not follow w1", cpu_block(), dict(OK, w2=torch.zeros(4, 3)), ValueError, "w2"),
    ("b1 bfloat16", cpu_block(), dict(OK, b1=torch.zeros(5, dtype=torch.bfloat16)), TypeError, "b1"),
    ("b1 of the length of b2", cpu_block(), dict(OK, b1=torch.zeros(3)), ValueError, "b1"),
    ("b2 of the length of b1", cpu_block(), dict(OK, b2=torch.zeros(5)), ValueError, "b2"),
    ("out of the wrong shape", cpu_block(), dict(OK, out=torch.zeros(2, 5)), ValueError, "out must be"),
    ("out against out_dtype", cpu_block(), dict(x=X.bfloat16(), w1=W1.bfloat16(), w2=W2.bfloat16(), out=torch.zeros(2, 3), out_dtype=torch.bfloat16),
     TypeError, "out_dtype"),
    ("a bfloat16 out of float32 operands", cpu_block(), dict(OK, out_dtype=torch.bfloat16), TypeError, "out_dtype"),
    ("fused=True outside the range", cpu_block(), dict(OK, w1=torch.zeros(4, 300), w2=torch.zeros(300, 3), fused=True), ValueError, "fused=True"),
    ("x on the host", cpu_block(), OK, ValueError, "device tensor"),
    ("x on the host, composition", cpu_block(), dict(OK, fused=False), ValueError, "device tensor"),
]


@pytest.mark.parametrize("what,blk,kw,exc,word", WRAPPER, ids=[w[0] for w in WRAPPER])
def test_wrapper_refusals_are_raised_before_device_work(what, blk, kw, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        blk.gin(**kw)
    with pytest.raises(exc, match=re.escape(word)):
        gnc.block_gin_run(blk, **kw)
