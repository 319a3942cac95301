"""CPU: gnnagg_block_rgcn_basis_run (include/gnnagg.h section F, "Block R-GCN layer, basis decomposition") without a device -- every
refusal of the C-ABI and of Block.rgcn_basis, each naming its argument and decided before any device work, and
gnnagg_block_rgcn_basis_supported at the edges of its rule."""
import re

import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

NAME = "gnnagg_block_rgcn_basis_run"
F32, B16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
# a call that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD = dict(ptr=0x1000, idx=0x2000, num_dst=4, src=0x3000, etype=0x3800, etype_eid=0x5000, val=0x4000, val_eid=0x5000, x=0x6000, x_dtype=B16,
            x_pitch=16, feat=16, w_self=0x7000, bases=0x8000, comp=0x8800, num_rel=50, num_bases=3, bias=0x9000, n_out=8, out=0xa000,
            out_dtype=B16, reduce=_lib.REDUCE_MEAN, flags=_lib.FLAG_RELU, stream=None)

REFUSALS = [
    ("negative num_dst", dict(num_dst=-1), "num_dst"),
    ("feat 0", dict(feat=0), "feat"),
    ("n_out 0", dict(n_out=0), "n_out"),
    ("num_rel 0", dict(num_rel=0), "num_rel"),
    ("num_bases 0", dict(num_bases=0), "num_bases"),
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
    ("bases past the LDS", dict(feat=128, x_pitch=128, n_out=64, num_rel=46, num_bases=7), "gnnagg_block_rgcn_basis_supported"),
    ("null blk_ptr", dict(ptr=None), "d_blk_ptr"),
    ("null etype", dict(etype=None, etype_eid=None), "d_etype"),
    ("null x", dict(x=None), "d_x"),
    ("null bases", dict(bases=None), "d_bases"),
    ("null comp", dict(comp=None), "d_comp"),
    ("null out", dict(out=None), "d_out"),
]


def call(**over):
    return gnc.lib().gnnagg_block_rgcn_basis_run(*dict(GOOD, **over).values())


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, over, word):
    assert call(**over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_num_dst_0_launches_nothing_and_still_refuses_what_is_wrong():
    nothing = dict.fromkeys(("ptr", "idx", "src", "etype", "etype_eid", "val", "val_eid", "x", "w_self", "bases", "comp", "bias", "out"))
    assert call(num_dst=0, **nothing) == _lib.OK
    assert call(num_dst=0, num_bases=0) == _lib.ERR_ARG


# the rule: feat, n_out <= 256, R >= 1, B >= 1 and 64 + 64 R (counts) + roundup16(4 R B) (comp) + tile (+ bf16: the image) <= 163840 bytes.
# fp32 256 columns, tile = 16 rows x (256 (B + 1) + 4) x 4 bytes: R = 40, B = 8 is 64 + 2560 + 1280 + 147712 = 151616, B = 9 has a tile of
# 164096 alone; with B = 8 the counts and comp take 96 R: R = 167 is 163808, R = 168 is 163904.  bf16 128 -> 64, pitch = 128 (B + 1) + 8
# elements, tile + image = (16 + 64) x 2 x pitch: R = 46, B = 6 is 64 + 2944 + 1104 + 144640 = 148752, B = 7 has 165120 of tile and image.
SUPPORTED = [(1, 1, 1, 1, F32, 1), (256, 256, 40, 8, F32, 1), (256, 256, 40, 9, F32, 0), (256, 256, 167, 8, F32, 1), (256, 256, 168, 8, F32, 0),
             (128, 64, 46, 6, B16, 1), (128, 64, 46, 7, B16, 0), (128, 64, 266, 8, F32, 1), (64, 64, 200, 8, B16, 1), (257, 1, 1, 1, F32, 0),
             (1, 257, 1, 1, F32, 0), (8, 8, 0, 1, F32, 0), (8, 8, 1, 0, B16, 0), (8, 8, -1, 1, B16, 0), (0, 8, 1, 1, F32, 0), (8, 0, 1, 1, B16, 0),
             (1, 1, 1 << 30, 1, F32, 0), (1, 1, 1, 1 << 30, F32, 0), (32, 16, 2, 2, 2, 0)]


@pytest.mark.parametrize("feat,n_out,num_rel,num_bases,dt,want", SUPPORTED)
def test_supported_at_the_edges_of_its_rule(feat, n_out, num_rel, num_bases, dt, want):
    L = gnc.lib()
    assert L.gnnagg_block_rgcn_basis_supported(feat, n_out, num_rel, num_bases, dt) == want
    if not want:
        assert L.gnnagg_block_rgcn_basis_grid_cap(feat, n_out, num_rel, num_bases, dt) == 0   # (inside the range the cap asks the device)
    if dt in (F32, B16):
        assert gnc.block_rgcn_basis_supported(feat, n_out, num_rel, num_bases, torch.float32 if dt == F32 else torch.bfloat16) == bool(want)


def test_many_relations_are_served_where_block_rgcn_says_no():
    assert gnc.lib().gnnagg_block_rgcn_basis_supported(128, 64, 266, 8, F32) == 1
    assert gnc.lib().gnnagg_block_rgcn_supported(128, 64, 266, F32) == 0


# ------------------------------------------------------------------------------------------------------------ the wrapper
i32 = lambda a: torch.tensor(a, dtype=torch.int32)
BLK = gnc.Block(i32([0, 2, 2]), i32([1, 0]), i32([5, 7]), None, 2, 2, 2)
X, V, C, T = torch.zeros(10, 4), torch.zeros(2, 4, 3), torch.zeros(5, 2), torch.zeros(2, dtype=torch.int32)
WRAPPER = [
    ("there is no max", dict(x=X, bases=V, comp=C, etype=T, reduce="max"), ValueError, "reduce"),
    ("etype_full without eid", dict(x=X, bases=V, comp=C, etype=T, etype_full=True), ValueError, "eid"),
    ("bases of another dtype", dict(x=X, bases=V.bfloat16(), comp=C, etype=T), TypeError, "bases"),
    ("bases 2-D", dict(x=X, bases=V[0], comp=C, etype=T), ValueError, "bases"),
    ("comp of another dtype", dict(x=X, bases=V, comp=C.double(), etype=T), TypeError, "comp"),
    ("comp with other columns", dict(x=X, bases=V, comp=torch.zeros(5, 3), etype=T), ValueError, "comp"),
    ("w_self of another shape", dict(x=X, bases=V, comp=C, etype=T, w_self=torch.zeros(4, 2)), ValueError, "w_self"),
    ("a bfloat16 out of float32 operands", dict(x=X, bases=V, comp=C, etype=T, out_dtype=torch.bfloat16), TypeError, "out_dtype"),
    ("fused=True outside the range", dict(x=torch.zeros(10, 300), bases=torch.zeros(2, 300, 3), comp=C, etype=T, fused=True), ValueError,
     "fused=True"),
    ("x on the host", dict(x=X, bases=V, comp=C, etype=T), ValueError, "device tensor"),
    ("x on the host, composition", dict(x=X, bases=V, comp=C, etype=T, fused=False), ValueError, "device tensor"),   # no CPU arm
]


@pytest.mark.parametrize("what,kw,exc,word", WRAPPER, ids=[w[0] for w in WRAPPER])
def test_wrapper_refusals_are_raised_before_device_work(what, kw, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        BLK.rgcn_basis(**kw)
    with pytest.raises(exc, match=re.escape(word)):
        gnc.block_rgcn_basis_run(BLK, **kw)
