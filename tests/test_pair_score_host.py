"""CPU: gnnagg_pair_score_run (include/gnnagg.h section G, "Pair scoring") without a device -- every refusal of the C-ABI and of
gnc.pair_score / Block.score, each naming its argument and decided before any device work, and gnnagg_pair_score_supported at the edges
of its rule."""
import re

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

NAME = "gnnagg_pair_score_run"
F32, B16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
DOT, MLP, MUL, CAT = _lib.PAIR_DOT, _lib.PAIR_MLP, _lib.PAIR_MUL, _lib.PAIR_CAT
# calls that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD_MLP = dict(kind=MLP, combine=CAT, u=0x1000, v=0x2000, ptr=None, idx=None, num_rows=0, num_pairs=5, src=0x3000, hu=0x4000, hu_pitch=16,
                hv=0x5000, hv_pitch=20, x_dtype=B16, feat=16, rel=None, etype=None, num_rel=0, w1=0x6000, b1=0x7000, hidden=24, w2=0x8000,
                b2=0x9000, n_out=8, out=0xa000, out_dtype=B16, flags=_lib.FLAG_RELU, stream=None)
GOOD_DOT = dict(GOOD_MLP, kind=DOT, combine=MUL, u=None, v=None, ptr=0x1000, idx=0x2000, num_rows=3, rel=0xb000, etype=0xc000, num_rel=4,
                w1=None, b1=None, hidden=0, w2=None, b2=None, n_out=0, out_dtype=F32, flags=0)

REFUSALS = [
    ("unknown kind", GOOD_MLP, dict(kind=2), "kind"),
    ("unknown combine", GOOD_MLP, dict(combine=2), "combine"),
    ("negative num_pairs", GOOD_MLP, dict(num_pairs=-1), "num_pairs"),
    ("feat 0", GOOD_MLP, dict(feat=0), "feat"),
    ("hu pitch below feat", GOOD_MLP, dict(hu_pitch=15), "hu_pitch"),
    ("hv pitch below feat", GOOD_MLP, dict(hv_pitch=15), "hv_pitch"),
    ("x dtype 2", GOOD_MLP, dict(x_dtype=2), "x_dtype"),
    ("x dtype 7", GOOD_DOT, dict(x_dtype=7), "x_dtype"),
    ("out dtype -1", GOOD_MLP, dict(out_dtype=-1), "out_dtype"),
    ("fp32 operands, bf16 out", GOOD_MLP, dict(x_dtype=F32), "out_dtype"),
    ("the accumulate flag", GOOD_MLP, dict(flags=_lib.FLAG_ACCUMULATE), "flags"),
    ("both pair forms", GOOD_MLP, dict(ptr=0x1000, idx=0x2000, num_rows=3), "both"),
    ("neither pair form", GOOD_MLP, dict(u=None, v=None), "neither"),
    ("u without v", GOOD_MLP, dict(v=None), "d_v"),
    ("ptr without idx", GOOD_DOT, dict(idx=None), "d_idx"),
    ("ptr of no rows", GOOD_DOT, dict(num_rows=0), "num_rows"),
    ("etype without rel", GOOD_DOT, dict(rel=None), "d_etype"),
    ("rel without etype", GOOD_DOT, dict(etype=None), "d_rel"),
    ("rel of no relations", GOOD_DOT, dict(num_rel=0), "num_rel"),
    ("w1 given to dot", GOOD_DOT, dict(w1=0x6000), "d_w1"),
    ("b2 given to dot", GOOD_DOT, dict(b2=0x6000), "d_b2"),
    ("dot with a bf16 out", GOOD_DOT, dict(out_dtype=B16), "out_dtype"),
    ("dot with the relu flag", GOOD_DOT, dict(flags=_lib.FLAG_RELU), "flags"),
    ("rel given to mlp", GOOD_MLP, dict(rel=0xb000, etype=0xc000, num_rel=4), "d_rel"),
    ("hidden 0", GOOD_MLP, dict(hidden=0), "hidden"),
    ("n_out 0", GOOD_MLP, dict(n_out=0), "n_out"),
    ("feat past the range", GOOD_MLP, dict(feat=257, hu_pitch=257, hv_pitch=257), "feat"),
    ("bf16 cat past the LDS", GOOD_MLP, dict(feat=256, hu_pitch=256, hv_pitch=256, hidden=256), "gnnagg_pair_score_supported"),
    ("null hu", GOOD_DOT, dict(hu=None), "d_hu"),
    ("null hv", GOOD_MLP, dict(hv=None), "d_hv"),
    ("null w1", GOOD_MLP, dict(w1=None), "d_w1"),
    ("null w2", GOOD_MLP, dict(w2=None), "d_w2"),
    ("null out", GOOD_DOT, dict(out=None), "d_out"),
]


def call(good, **over):
    return gnc.lib().gnnagg_pair_score_run(*dict(good, **over).values())


@pytest.mark.parametrize("what,good,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, good, over, word):
    assert call(good, **over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_no_pairs_launch_nothing_and_still_refuse_what_is_wrong():
    nothing = dict(num_pairs=0, u=None, v=None, ptr=None, idx=None, src=None, hu=None, hv=None, out=None)
    assert call(GOOD_MLP, w1=None, b1=None, w2=None, b2=None, **nothing) == _lib.OK
    assert call(GOOD_DOT, rel=None, etype=None, **nothing) == _lib.OK
    assert call(GOOD_MLP, num_pairs=0, hidden=0) == _lib.ERR_ARG
    assert call(GOOD_DOT, num_pairs=0, w2=0x6000) == _lib.ERR_ARG


# mlp, tiles of 32 pairs.  bf16: 64 (Kp + 8) + 64 (Hp + 8) + 2 roundup16(hidden) (Kp + 8) + 2 roundup16(n_out) (Hp + 8) bytes against 163 840,
# Kp = the k of W1 (feat, cat: 2 feat) and Hp = hidden rounded up to 32: mul 256 -> 256 -> 16 is 177 408, mul 256 -> 128 -> 256 is 162 816
# and mul 256 -> 144 -> 256 (Hp = 160) 189 696, cat 128 -> 128 -> 47 is 106 240; cat 256 -> 256: the image of W1 alone is 266 240.
# fp32 (no image) cat 256 -> 256 -> 256: 32 * 516 * 4 + 32 * 260 * 4 = 99 328.
SUPPORTED = [(MLP, MUL, 1, 1, 1, F32, 1), (MLP, CAT, 256, 256, 256, F32, 1), (MLP, MUL, 257, 1, 1, F32, 0), (MLP, MUL, 1, 257, 1, F32, 0),
             (MLP, CAT, 1, 1, 257, F32, 0), (MLP, MUL, 0, 8, 8, F32, 0), (MLP, MUL, 8, 0, 8, B16, 0), (MLP, CAT, 8, 8, 0, B16, 0),
             (MLP, MUL, 256, 128, 256, B16, 1), (MLP, MUL, 256, 144, 256, B16, 0), (MLP, MUL, 256, 256, 16, B16, 0),
             (MLP, CAT, 128, 128, 47, B16, 1), (MLP, CAT, 256, 256, 1, B16, 0), (MLP, MUL, 128, 128, 128, 2, 0), (MLP, MUL, 128, 128, 128, -1, 0),
             (MLP, 2, 8, 8, 8, F32, 0), (2, MUL, 8, 8, 8, F32, 0), (DOT, MUL, 1, 0, 0, F32, 1), (DOT, MUL, 100000, 0, 0, B16, 1),
             (DOT, MUL, 0, 0, 0, F32, 0), (DOT, MUL, 64, 0, 0, 2, 0), (DOT, MUL, 64, 0, 0, -1, 0)]


@pytest.mark.parametrize("kind,combine,feat,hidden,n_out,dt,want", SUPPORTED)
def test_supported_at_the_edges_of_its_rule(kind, combine, feat, hidden, n_out, dt, want):
    L = gnc.lib()
    assert L.gnnagg_pair_score_supported(kind, combine, feat, hidden, n_out, dt) == want
    assert (L.gnnagg_pair_score_grid_cap(kind, combine, feat, hidden, n_out, dt) == 0) == (not want)
    if dt in (F32, B16) and kind in (DOT, MLP) and combine in (MUL, CAT):
        tdt = torch.float32 if dt == F32 else torch.bfloat16
        assert gnc.pair_score_supported("dot" if kind == DOT else "mlp", "cat" if combine == CAT else "mul", feat, hidden, n_out, tdt) == bool(want)


# ------------------------------------------------------------------------------------------------------------ the wrapper
i32 = lambda a: torch.tensor(a, dtype=torch.int32)
H, W1, W2, U, V = torch.zeros(10, 4), torch.zeros(4, 5), torch.zeros(5, 3), i32([0, 1, 1]), i32([2, 2, 3])
COO = dict(hu=H, hv=H, u=U, v=V)
OK_MLP = dict(COO, kind="mlp", w1=W1, w2=W2)
WRAPPER = [
    ("unknown kind", dict(COO, kind="cos"), ValueError, "kind"),
    ("unknown combine", dict(OK_MLP, combine="sum"), ValueError, "combine"),
    ("out_dtype float16", dict(COO, out_dtype=torch.float16), TypeError, "out_dtype"),
    ("both pair forms", dict(COO, ptr=i32([0, 3]), idx=V), ValueError, "both"),
    ("neither pair form", dict(hu=H, hv=H), ValueError, "neither"),
    ("u without v", dict(hu=H, hv=H, u=U), TypeError, "v must be"),
    ("idx int64", dict(hu=H, hv=H, ptr=i32([0, 3]), idx=V.long()), TypeError, "idx must be"),
    ("u and v of two lengths", dict(COO, v=i32([1])), ValueError, "one length"),
    ("src float", dict(COO, src=torch.zeros(4)), TypeError, "src"),
    ("hu float16", dict(COO, hu=H.half()), TypeError, "hu must be"),
    ("hv of another dtype", dict(COO, hv=H.bfloat16()), TypeError, "hv"),
    ("hu 1-D", dict(COO, hu=torch.zeros(10)), ValueError, "2-D"),
    ("hv of another width", dict(COO, hv=torch.zeros(10, 5)), ValueError, "hv"),
    ("etype without rel", dict(COO, etype=i32([0, 0, 0])), ValueError, "rel"),
    ("rel without etype", dict(COO, rel=torch.zeros(2, 4)), ValueError, "etype"),
    ("rel bfloat16", dict(COO, rel=torch.zeros(2, 4, dtype=torch.bfloat16), etype=i32([0, 0, 0])), TypeError, "rel"),
    ("rel of another width", dict(COO, rel=torch.zeros(2, 5), etype=i32([0, 0, 0])), ValueError, "rel"),
    ("etype of another length", dict(COO, rel=torch.zeros(2, 4), etype=i32([0, 0])), ValueError, "etype"),
    ("weights given to dot", dict(COO, w1=W1), ValueError, "w1"),
    ("relu given to dot", dict(COO, relu=True), ValueError, "mlp"),
    ("a bfloat16 out of dot", dict(COO, out_dtype=torch.bfloat16), TypeError, "out_dtype"),
    ("rel given to mlp", dict(OK_MLP, rel=torch.zeros(2, 4), etype=i32([0, 0, 0])), ValueError, "dot"),
    ("w1 no tensor", dict(OK_MLP, w1=np.zeros((4, 5), np.float32)), TypeError, "w1"),
    ("w1 of mul under cat", dict(OK_MLP, combine="cat"), ValueError, "w1"),
    ("w2 that does not follow w1", dict(OK_MLP, w2=torch.zeros(4, 3)), ValueError, "w2"),
    ("b1 of the length of b2", dict(OK_MLP, b1=torch.zeros(3)), ValueError, "b1"),
    ("b2 bfloat16", dict(OK_MLP, b2=torch.zeros(3, dtype=torch.bfloat16)), TypeError, "b2"),
    ("out of the wrong shape", dict(OK_MLP, out=torch.zeros(3, 5)), ValueError, "out must be"),
    ("a bfloat16 out of float32 operands", dict(OK_MLP, out_dtype=torch.bfloat16), TypeError, "out_dtype"),
    ("fused=True outside the range", dict(OK_MLP, w1=torch.zeros(4, 300), w2=torch.zeros(300, 3), fused=True), ValueError, "fused=True"),
    ("hu on the host", COO, ValueError, "device tensor"),
    ("hu on the host, composition", dict(OK_MLP, fused=False), ValueError, "device tensor"),
]


@pytest.mark.parametrize("what,kw,exc,word", WRAPPER, ids=[w[0] for w in WRAPPER])
def test_wrapper_refusals_are_raised_before_device_work(what, kw, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        gnc.pair_score(**kw)


def test_block_score_passes_its_own_csr_and_refuses_the_same():
    blk = gnc.Block(i32([0, 2, 2]), i32([1, 0]), i32([5, 7]), None, 2, 2, 2)
    with pytest.raises(ValueError, match="etype must be \\[2\\]"):
        blk.score(H, rel=torch.zeros(2, 4), etype=i32([0, 0, 0]))
    with pytest.raises(ValueError, match="device tensor"):
        blk.score(H, kind="mlp", w1=W1, w2=W2, gathered=True)
