"""CPU: gnnagg_block_pna_run (include/gnnagg.h section F, "Block PNA layer") without a device -- every refusal of the C-ABI and of
Block.pna, each naming its argument and decided before any device work, and gnnagg_block_pna_supported on both sides of its LDS rule."""
import re

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

NAME = "gnnagg_block_pna_run"
F32, B16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
# a call that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD = dict(ptr=0x1000, idx=0x2000, num_dst=4, src=0x3000, val=0x4000, eid=0x5000, x=0x6000, x_dtype=B16, x_pitch=16, feat=16,
            aggr_mask=_lib.AGGR_MEAN | _lib.AGGR_MAX | _lib.AGGR_STD, scaler_mask=_lib.SCALER_IDENTITY | _lib.SCALER_ATTENUATION, delta=1.5,
            w_self=0x7000, w=0x8000, bias=0x9000, n_out=8, out=0xa000, out_dtype=B16, flags=_lib.FLAG_RELU, stream=None)

REFUSALS = [
    ("negative num_dst", dict(num_dst=-1), "num_dst"),
    ("feat 0", dict(feat=0), "feat"),
    ("n_out 0", dict(n_out=0), "n_out"),
    ("pitch below feat", dict(x_pitch=15), "x_pitch"),
    ("unknown x dtype", dict(x_dtype=2), "x_dtype"),
    ("unknown out dtype", dict(out_dtype=-1), "out_dtype"),
    ("fp32 operands, bf16 out", dict(x_dtype=F32), "out_dtype"),
    ("no aggregate", dict(aggr_mask=0), "aggr_mask"),
    ("an unknown aggregate bit", dict(aggr_mask=64), "aggr_mask"),
    ("no scaler", dict(scaler_mask=0), "scaler_mask"),
    ("an unknown scaler bit", dict(scaler_mask=8), "scaler_mask"),
    ("attenuation with delta 0", dict(delta=0.0), "delta"),
    ("attenuation with a negative delta", dict(delta=-1.0), "delta"),
    ("amplification with a NaN delta", dict(scaler_mask=_lib.SCALER_AMPLIFICATION, delta=float("nan")), "delta"),
    ("amplification with an infinite delta", dict(scaler_mask=_lib.SCALER_AMPLIFICATION, delta=float("inf")), "delta"),
    ("the accumulate flag", dict(flags=_lib.FLAG_ACCUMULATE), "flags"),
    ("eid without val", dict(val=None), "d_eid"),
    ("feat past the range", dict(feat=257, x_pitch=257), "gnnagg_block_pna_supported"),
    ("n_out past the range", dict(n_out=257), "gnnagg_block_pna_supported"),
    ("a bf16 image past the LDS", dict(feat=128, x_pitch=128, n_out=64, aggr_mask=15, scaler_mask=7), "gnnagg_block_pna_supported"),
    ("null blk_ptr", dict(ptr=None), "d_blk_ptr"),
    ("null x", dict(x=None), "d_x"),
    ("null w", dict(w=None), "d_w"),
    ("null out", dict(out=None), "d_out"),
]


def call(**over):
    return gnc.lib().gnnagg_block_pna_run(*dict(GOOD, **over).values())


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, over, word):
    assert call(**over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_num_dst_0_launches_nothing_and_still_refuses_what_is_wrong():
    assert call(num_dst=0, ptr=None, idx=None, x=None, w_self=None, w=None, bias=None, out=None, src=None, val=None, eid=None) == _lib.OK
    assert call(num_dst=0, scaler_mask=_lib.SCALER_IDENTITY, delta=float("nan")) == _lib.OK      # identity alone never reads delta
    assert call(num_dst=0, aggr_mask=0) == _lib.ERR_ARG


# bytes against 163 840, Fp = feat rounded up to 4 (fp32) / 32 (bf16): fp32 192 + 64 (roundup8((1 + A) Fp) + 4), 256 columns x 6 aggregates
# 115 136; bf16 192 + 32 ((1 + A) Fp + 8) + 2 roundup16(n_out) ((1 + S A) Fp + 8): 128 -> 64 with 4 x 1 is 103 872, with 4 x 3 234 944;
# 64 -> 64 with 4 x 3 is 118 208; 100 -> 128 with 3 x 1 is 149 952 and with 4 x 1 186 816; 128 -> 96 with 4 x 1 is 145 344, -> 97 (112
# image rows) 166 080.
SUPPORTED = [(1, 1, 1, 1, F32, 1), (256, 256, 6, 3, F32, 1), (257, 1, 1, 1, F32, 0), (1, 257, 1, 1, F32, 0), (0, 8, 1, 1, F32, 0),
             (8, 0, 1, 1, B16, 0), (8, 8, 0, 1, F32, 0), (8, 8, 7, 1, F32, 0), (8, 8, 1, 0, B16, 0), (8, 8, 1, 4, B16, 0),
             (128, 64, 4, 1, B16, 1), (128, 64, 4, 3, B16, 0), (64, 64, 4, 3, B16, 1), (100, 128, 3, 1, B16, 1), (100, 128, 4, 1, B16, 0),
             (128, 96, 4, 1, B16, 1), (128, 97, 4, 1, B16, 0), (128, 64, 4, 1, 2, 0)]


@pytest.mark.parametrize("feat,n_out,n_aggr,n_scaler,dt,want", SUPPORTED)
def test_supported_on_both_sides_of_its_rule(feat, n_out, n_aggr, n_scaler, dt, want):
    L = gnc.lib()
    assert L.gnnagg_block_pna_supported(feat, n_out, n_aggr, n_scaler, dt) == want
    if not want:
        assert L.gnnagg_block_pna_grid_cap(feat, n_out, n_aggr, n_scaler, dt) == 0   # (inside the range the cap asks the device for its CUs)
    if dt in (F32, B16):
        assert gnc.block_pna_supported(feat, n_out, n_aggr, n_scaler, torch.float32 if dt == F32 else torch.bfloat16) == bool(want)


# ------------------------------------------------------------------------------------------------------------ the wrapper
def cpu_block(eid=False, relabel=True):
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return gnc.Block(i32([0, 2, 2]), i32([1, 0]), i32([5, 7]) if relabel else None, i32([3, 9]) if eid else None, 2, 2 if relabel else 10, 2)


X, W, WS = torch.zeros(10, 4), torch.zeros(16, 3), torch.zeros(4, 3)
OK = dict(x=X, w=W)
WRAPPER = [
    ("an unknown aggregate", dict(OK, aggrs=("mean", "median")), ValueError, "aggrs"),
    ("an aggregate twice", dict(OK, aggrs=("mean", "mean")), ValueError, "aggrs"),
    ("no scaler", dict(OK, scalers=()), ValueError, "scalers"),
    ("attenuation without delta", dict(OK, w=torch.zeros(32, 3), scalers=("identity", "attenuation")), ValueError, "delta"),
    ("amplification with delta 0", dict(OK, scalers="amplification", delta=0.0), ValueError, "delta"),
    ("val_full without eid", dict(OK, val=torch.zeros(20), val_full=True), ValueError, "eid"),
    ("out_dtype float16", dict(OK, out_dtype=torch.float16), TypeError, "out_dtype"),
    ("x float16", dict(x=X.half(), w=W.half()), TypeError, "x must be"),
    ("x 1-D", dict(OK, x=torch.zeros(10)), ValueError, "2-D"),
    ("a gathered x with too few rows", dict(OK, x=torch.zeros(1, 4), gathered=True), ValueError, "rows"),
    ("val of the wrong length", dict(OK, val=torch.zeros(3)), ValueError, "val"),
    ("w no tensor", dict(OK, w=np.zeros((16, 3), np.float32)), TypeError, "w must be"),
    ("w for another number of slabs", dict(OK, aggrs=("mean", "max")), ValueError, "S * A * F"),
    ("w_self of another dtype", dict(OK, w_self=WS.bfloat16()), TypeError, "w_self"),
    ("w_self with other columns", dict(OK, w_self=torch.zeros(4, 5)), ValueError, "w_self"),
    ("bias bfloat16", dict(OK, bias=torch.zeros(3, dtype=torch.bfloat16)), TypeError, "bias"),
    ("bias of the wrong length", dict(OK, bias=torch.zeros(4)), ValueError, "bias"),
    ("out of the wrong shape", dict(OK, out=torch.zeros(2, 5)), ValueError, "out must be"),
    ("a bfloat16 out of float32 operands", dict(OK, out_dtype=torch.bfloat16), TypeError, "out_dtype"),
    ("fused=True outside the range", dict(OK, w=torch.zeros(16, 300), fused=True), ValueError, "fused=True"),
    ("x on the host", OK, ValueError, "device tensor"),
    ("x on the host, composition", dict(OK, fused=False), ValueError, "device tensor"),
]


@pytest.mark.parametrize("what,kw,exc,word", WRAPPER, ids=[w[0] for w in WRAPPER])
def test_wrapper_refusals_are_raised_before_device_work(what, kw, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        cpu_block().pna(**kw)
    with pytest.raises(exc, match=re.escape(word)):
        gnc.block_pna_run(cpu_block(), **kw)
