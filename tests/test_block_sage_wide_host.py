"""CPU: gnnagg_block_sage_wide_run (include/gnnagg.h section F, "Block SAGE layer, wide rows") without a device -- the refusals of the
C-ABI and of Block.sage(fused="wide"), each before any device work; gnnagg_block_sage_wide_supported at the edges of its rule; and the
condition that the LDS of a workgroup does not grow with feat: a grid cap constant in feat, two workgroups per CU and more at every shape."""
import re

import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

NAME = "gnnagg_block_sage_wide_run"
F32, B16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
# a call that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD = dict(ptr=0x1000, idx=0x2000, num_dst=4, src=0x3000, val=0x4000, eid=0x5000, x=0x6000, x_dtype=B16, x_pitch=608, feat=602, w_self=0x7000,
            w_neigh=0x8000, bias=0x9000, n_out=128, out=0xa000, out_dtype=B16, reduce=_lib.REDUCE_MEAN, flags=_lib.FLAG_RELU, stream=None)

REFUSALS = [
    ("negative num_dst", dict(num_dst=-1), "num_dst"),
    ("feat 0", dict(feat=0), "feat"),
    ("n_out 0", dict(n_out=0), "n_out"),
    ("pitch below feat", dict(x_pitch=601), "x_pitch"),
    ("unknown x dtype", dict(x_dtype=2), "x_dtype"),
    ("unknown out dtype", dict(out_dtype=-1), "out_dtype"),
    ("fp32 operands, bf16 out", dict(x_dtype=F32), "out_dtype"),
    ("unknown reduce", dict(reduce=3), "reduce"),
    ("the accumulate flag", dict(flags=_lib.FLAG_ACCUMULATE), "flags"),
    ("eid without val", dict(val=None), "d_eid"),
    ("feat past the range", dict(feat=4097, x_pitch=4097), "gnnagg_block_sage_wide_supported"),
    ("n_out past the range", dict(n_out=257), "gnnagg_block_sage_wide_supported"),
    ("null blk_ptr", dict(ptr=None), "d_blk_ptr"),
    ("null x", dict(x=None), "d_x"),
    ("null w_neigh", dict(w_neigh=None), "d_w_neigh"),
    ("null out", dict(out=None), "d_out"),
]


def call(**over):
    return gnc.lib().gnnagg_block_sage_wide_run(*dict(GOOD, **over).values())


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, over, word):
    assert call(**over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_num_dst_0_launches_nothing_and_still_refuses_what_is_wrong():
    assert call(num_dst=0, ptr=None, idx=None, x=None, w_self=None, w_neigh=None, bias=None, out=None, src=None, val=None, eid=None) == _lib.OK
    assert call(num_dst=0, n_out=0) == _lib.ERR_ARG


@pytest.mark.parametrize("feat,n_out,dt,want", [(1, 1, F32, 1), (4096, 256, F32, 1), (4097, 1, F32, 0), (1, 257, F32, 0), (0, 8, F32, 0),
                                                (1, 1, B16, 1), (4096, 256, B16, 1), (4097, 1, B16, 0), (1, 257, B16, 0), (602, 128, 2, 0),
                                                (602, 128, -1, 0)])
def test_supported_at_the_edges_of_its_rule(feat, n_out, dt, want):
    L = gnc.lib()
    assert L.gnnagg_block_sage_wide_supported(feat, n_out, dt) == want
    if not want:
        assert L.gnnagg_block_sage_wide_grid_cap(feat, n_out, dt) == 0
    if dt in (F32, B16):
        assert gnc.block_sage_wide_supported(feat, n_out, torch.float32 if dt == F32 else torch.bfloat16) == bool(want)
    else:
        assert L.gnnagg_block_sage_wide_chunk(dt) == 0


@pytest.mark.parametrize("dt,kblock", [(F32, 4), (B16, 32)], ids=["fp32", "bf16"])
def test_the_grid_cap_is_constant_in_feat_and_two_workgroups_fit_a_cu(dt, kblock):
    L = gnc.lib()
    kc = L.gnnagg_block_sage_wide_chunk(dt)
    assert kc > 0 and kc % kblock == 0                       # whole MFMA k blocks
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256   # (no device: the library says 256)
    for n_out in (1, 17, 128, 129, 256):
        caps = {L.gnnagg_block_sage_wide_grid_cap(feat, n_out, dt) for feat in (1, kc, kc + 1, 602, 1024, 4096)}
        assert len(caps) == 1 and caps.pop() >= 2 * cus, n_out


def cpu_block():
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return gnc.Block(i32([0, 2, 2]), i32([1, 0]), i32([5, 7]), None, 2, 2, 2)


WRAPPER = [
    ("feat past the range", dict(x=torch.zeros(10, 4097), w_neigh=torch.zeros(4097, 3), fused="wide"), ValueError, "gnnagg_block_sage_wide_supported"),
    ("n_out past the range", dict(x=torch.zeros(10, 602), w_neigh=torch.zeros(602, 257), fused="wide"), ValueError, "gnnagg_block_sage_wide_supported"),
    ("x on the host", dict(x=torch.zeros(10, 602), w_neigh=torch.zeros(602, 3), fused="wide"), ValueError, "device tensor"),
]


@pytest.mark.parametrize("what,kw,exc,word", WRAPPER, ids=[w[0] for w in WRAPPER])
def test_wrapper_refusals_are_raised_before_device_work(what, kw, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        cpu_block().sage(**kw)
    with pytest.raises(exc, match=re.escape(word)):
        gnc.block_sage_run(cpu_block(), **kw)
