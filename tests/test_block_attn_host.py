"""CPU: gnnagg_block_attn_run (include/gnnagg.h section F, "Block attention") without a device -- every refusal of the C-ABI and of
Block.attend, each naming its argument and decided before any device work."""
import re

import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

NAME = "gnnagg_block_attn_run"
F32, B16, DOT, V2 = _lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.ATTN_DOT, _lib.ATTN_GATV2
# a call that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD = dict(ptr=0x1000, idx=0x2000, num_dst=4, src=0x3000, eid=0x4000, kind=DOT, q=0x5000, q_pitch=48, k=0x6000, v=0x7000, kv_pitch=48, a=None,
            slope=0.2, scale=0.25, bias=0x8000, bias_heads=2, ef=0x9000, ef_pitch=16, x_dtype=B16, y=0xa000, y_dtype=F32, feat=16, heads=2,
            stream=None)
GATV2 = dict(kind=V2, v=None, a=0xb000)

REFUSALS = [
    ("negative num_dst", dict(num_dst=-1), "num_dst"),
    ("unknown kind", dict(kind=2), "kind"),
    ("unknown x dtype", dict(x_dtype=2), "x_dtype"),
    ("unknown y dtype", dict(y_dtype=-1), "y_dtype"),
    ("heads not dividing feat", dict(heads=3), "heads"),
    ("feat above the limit", dict(feat=1026, q_pitch=1026, kv_pitch=1026, ef_pitch=1026), "feat"),
    ("q pitch below feat", dict(q_pitch=15), "q_pitch"),
    ("kv pitch below feat", dict(kv_pitch=15), "kv_pitch"),
    ("ef pitch below feat", dict(ef_pitch=15), "ef_pitch"),
    ("infinite scale", dict(scale=float("inf")), "scale"),
    ("NaN scale", dict(scale=float("nan")), "scale"),
    ("slope above 1", dict(GATV2, slope=1.5), "slope"),
    ("bias_heads neither 1 nor heads", dict(bias_heads=4), "bias_heads"),
    ("eid with neither bias nor ef", dict(bias=None, ef=None), "d_eid"),
    ("v given for GATv2", dict(GATV2, v=0x7000), "d_v"),
    ("v missing for dot", dict(v=None), "d_v"),
    ("a missing for GATv2", dict(GATV2, a=None), "d_a"),
    ("null blk_ptr", dict(ptr=None), "d_blk_ptr"),
    ("null q", dict(q=None), "d_q"),
    ("null k", dict(k=None), "d_k"),
    ("null y", dict(y=None), "d_y"),
]


def call(**over):
    return gnc.lib().gnnagg_block_attn_run(*dict(GOOD, **over).values())


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, over, word):
    assert call(**over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_num_dst_0_launches_nothing_and_still_refuses_what_is_wrong():
    nothing = dict(num_dst=0, ptr=None, idx=None, src=None, eid=None, q=None, k=None, v=None, bias=None, ef=None, y=None)
    assert call(**nothing) == _lib.OK
    assert call(**dict(nothing, **GATV2)) == _lib.OK
    assert call(num_dst=0, heads=3) == _lib.ERR_ARG
    assert call(**dict(nothing, v=0x7000, kind=V2)) == _lib.ERR_ARG


# ------------------------------------------------------------------------------------------------------------ the wrapper
def cpu_block(eid=False, relabel=True):
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return gnc.Block(i32([0, 2, 2]), i32([1, 0]), i32([5, 7]) if relabel else None, i32([3, 9]) if eid else None, 2, 2 if relabel else 10, 2)


X, A = torch.zeros(10, 4), torch.zeros(4)
WRAPPER = [
    ("unknown kind", cpu_block(), dict(q=X, k=X, v=X, kind="gat"), ValueError, "kind"),
    ("bias_full without eid", cpu_block(), dict(q=X, k=X, v=X, bias=torch.zeros(20), bias_full=True), ValueError, "eid"),
    ("edge_full without eid", cpu_block(), dict(q=X, k=X, v=X, edge=torch.zeros(20, 4), edge_full=True), ValueError, "eid"),
    ("bias_full without bias", cpu_block(eid=True), dict(q=X, k=X, v=X, bias_full=True), ValueError, "bias"),
    ("bias per block edge beside full edge rows", cpu_block(eid=True),
     dict(q=X, k=X, v=X, bias=torch.zeros(2), edge=torch.zeros(20, 4), edge_full=True), ValueError, "one eid"),
    ("dot without v", cpu_block(), dict(q=X, k=X), ValueError, "needs v"),
    ("gatv2 with v", cpu_block(), dict(q=X, k=X, v=X, kind="gatv2", a=A), ValueError, "v must be None"),
    ("gatv2 without a", cpu_block(), dict(q=X, k=X, kind="gatv2"), TypeError, "needs a"),
    ("a of the wrong size", cpu_block(), dict(q=X, k=X, kind="gatv2", a=torch.zeros(3)), ValueError, "a (3,)"),
    ("slope outside [0, 1]", cpu_block(), dict(q=X, k=X, kind="gatv2", a=A, slope=-0.1), ValueError, "slope"),
    ("out_dtype float16", cpu_block(), dict(q=X, k=X, v=X, out_dtype=torch.float16), TypeError, "out_dtype"),
    ("q float16", cpu_block(), dict(q=X.half(), k=X.half(), v=X.half()), TypeError, "q must be"),
    ("k of another dtype", cpu_block(), dict(q=X, k=X.bfloat16(), v=X), TypeError, "k ("),
    ("q 1-D", cpu_block(), dict(q=torch.zeros(10), k=X, v=X), ValueError, "2-D"),
    ("heads not dividing F", cpu_block(), dict(q=X, k=X, v=X, heads=3), ValueError, "heads"),
    ("F above the limit", cpu_block(), dict(q=torch.zeros(10, 1026), k=torch.zeros(10, 1026), v=torch.zeros(10, 1026)), ValueError, "limit"),
    ("k with other columns", cpu_block(), dict(q=X, k=torch.zeros(10, 8), v=torch.zeros(10, 8)), ValueError, "columns"),
    ("k and v of two pitches", cpu_block(), dict(q=X, k=X, v=torch.zeros(10, 8)[:, :4]), ValueError, "row pitch"),
    ("gathered operands with too few rows", cpu_block(), dict(q=X, k=torch.zeros(1, 4), v=torch.zeros(1, 4), gathered=True), ValueError, "rows"),
    ("an infinite scale", cpu_block(), dict(q=X, k=X, v=X, scale=float("inf")), ValueError, "scale"),
    ("bias of the wrong length", cpu_block(), dict(q=X, k=X, v=X, bias=torch.zeros(3)), ValueError, "bias"),
    ("bias bfloat16", cpu_block(), dict(q=X, k=X, v=X, bias=torch.zeros(2, dtype=torch.bfloat16)), TypeError, "bias"),
    ("edge of the wrong shape", cpu_block(), dict(q=X, k=X, v=X, edge=torch.zeros(2, 3)), ValueError, "edge"),
    ("edge of another dtype", cpu_block(), dict(q=X, k=X, v=X, edge=torch.zeros(2, 4, dtype=torch.bfloat16)), TypeError, "edge"),
    ("out of the wrong shape", cpu_block(), dict(q=X, k=X, v=X, out=torch.zeros(3, 4)), ValueError, "out must be"),
    ("out against out_dtype", cpu_block(), dict(q=X, k=X, v=X, out=torch.zeros(2, 4), out_dtype=torch.bfloat16), TypeError, "out_dtype"),
    ("q on the host", cpu_block(), dict(q=X, k=X, v=X), ValueError, "device tensor"),
]


@pytest.mark.parametrize("what,blk,kw,exc,word", WRAPPER, ids=[w[0] for w in WRAPPER])
def test_wrapper_refusals_are_raised_before_the_library_is_reached(what, blk, kw, exc, word, monkeypatch):
    def unreachable():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(gnc.sampling, "lib", unreachable)
    with pytest.raises(exc, match=re.escape(word)):
        blk.attend(**kw)
    with pytest.raises(exc, match=re.escape(word)):
        gnc.block_attn_run(blk, **kw)
