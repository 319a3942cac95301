"""CPU: gnnagg_block_edgeconv_run (include/gnnagg.h section H, "Block EdgeConv layer") without a device -- every refusal of the C-ABI and
of Block.edgeconv, each naming its argument and decided before any device work, and gnnagg_block_edgeconv_supported at the edges of its rule."""
import re

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

NAME = "gnnagg_block_edgeconv_run"
F32, B16 = _lib.DTYPE_F32, _lib.DTYPE_BF16
DIFF, CAT = _lib.EDGECONV_DIFF, _lib.EDGECONV_CAT
# a call that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD = dict(ptr=0x1000, idx=0x2000, num_dst=4, src=0x3000, x=0x6000, x_dtype=B16, x_pitch=16, feat=16, combine=DIFF, w1=0x7000, b1=0x8000,
            hidden=24, w2=0x9000, b2=0xa000, n_out=8, out=0xb000, out_dtype=B16, reduce=_lib.REDUCE_MAX, flags=_lib.FLAG_RELU, stream=None)

REFUSALS = [
    ("negative num_dst", dict(num_dst=-1), "num_dst"),
    ("unknown combine", dict(combine=2), "combine"),
    ("unknown reduce", dict(reduce=3), "reduce"),
    ("feat 0", dict(feat=0), "feat"),
    ("hidden 0", dict(hidden=0), "hidden"),
    ("n_out 0", dict(n_out=0), "n_out"),
    ("pitch below feat", dict(x_pitch=15), "x_pitch"),
    ("unknown x dtype", dict(x_dtype=2), "x_dtype"),
    ("unknown out dtype", dict(out_dtype=-1), "out_dtype"),
    ("fp32 operands, bf16 out", dict(x_dtype=F32), "out_dtype"),
    ("the accumulate flag", dict(flags=_lib.FLAG_ACCUMULATE), "flags"),
    ("feat past the range", dict(feat=257, x_pitch=257), "feat"),
    ("hidden past the range", dict(hidden=257), "hidden"),
    ("n_out past the range", dict(n_out=257), "n_out"),
    ("bf16 images past the LDS", dict(feat=128, x_pitch=128, hidden=256, n_out=256), "gnnagg_block_edgeconv_supported"),
    ("null blk_ptr", dict(ptr=None), "d_blk_ptr"),
    ("null x", dict(x=None), "d_x"),
    ("null w1", dict(w1=None), "d_w1"),
    ("null w2", dict(w2=None), "d_w2"),
    ("null out", dict(out=None), "d_out"),
]


def call(**over):
    return gnc.lib().gnnagg_block_edgeconv_run(*dict(GOOD, **over).values())


def test_the_signature_is_typed():
    assert len(_lib.SIGNATURES[NAME][1]) == len(GOOD) and gnc.lib().gnnagg_block_edgeconv_run.argtypes is not None


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, over, word):
    assert call(**over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_num_dst_0_launches_nothing_and_still_refuses_what_is_wrong():
    assert call(num_dst=0, ptr=None, idx=None, x=None, w1=None, b1=None, w2=None, b2=None, out=None, src=None) == _lib.OK
    assert call(num_dst=0, hidden=0) == _lib.ERR_ARG


# bytes against 163 840, with Kp / Hp = 2 feat / hidden rounded up to 32 (bf16) and pn = roundup16(n_out) + 4:
#   384 + 64 pn + max(64 (Kp + 8), 128 pn) + 64 (Hp + 8) + 2 roundup16(hidden) (Kp + 8) + 2 roundup16(n_out) (Hp + 8)
# bf16 64 -> 64 -> 128 is 66 176; 128 -> 192 -> 64 is 161 408 and -> 65 (80 image rows, pn = 84) 168 832; 128 -> 256 -> 256 is 337 536.
# fp32 (no images, 4-byte tiles) 256 -> 256 -> 256: 384 + 16 640 + 66 048 + 33 280 = 116 352.
SUPPORTED = [(DIFF, 1, 1, 1, F32, 1), (CAT, 256, 256, 256, F32, 1), (DIFF, 257, 1, 1, F32, 0), (CAT, 1, 257, 1, F32, 0), (DIFF, 1, 1, 257, F32, 0),
             (DIFF, 0, 8, 8, F32, 0), (CAT, 8, 0, 8, B16, 0), (CAT, 8, 8, 0, B16, 0), (2, 8, 8, 8, F32, 0), (-1, 8, 8, 8, B16, 0),
             (DIFF, 64, 64, 128, B16, 1), (CAT, 128, 192, 64, B16, 1), (CAT, 128, 192, 65, B16, 0), (DIFF, 128, 256, 256, B16, 0),
             (DIFF, 128, 256, 256, F32, 1), (DIFF, 8, 8, 8, 2, 0)]


@pytest.mark.parametrize("combine,feat,hidden,n_out,dt,want", SUPPORTED)
def test_supported_at_the_edges_of_its_rule_and_equal_to_what_run_refuses(combine, feat, hidden, n_out, dt, want):
    L = gnc.lib()
    assert L.gnnagg_block_edgeconv_supported(combine, feat, hidden, n_out, dt) == want
    if not want:
        assert L.gnnagg_block_edgeconv_grid_cap(combine, feat, hidden, n_out, dt) == 0   # (inside the range the cap asks the device for its CUs)
    # num_dst = 0 stops after the checks: OK exactly where the shape is served (a bf16 out of fp32 operands is a refusal of its own)
    rc = call(num_dst=0, combine=combine, feat=feat, x_pitch=max(feat, 1), hidden=hidden, n_out=n_out, x_dtype=dt, out_dtype=dt)
    assert rc == (_lib.OK if want else _lib.ERR_ARG)
    if dt in (F32, B16) and combine in (DIFF, CAT):
        name = "diff" if combine == DIFF else "cat"
        assert gnc.block_edgeconv_supported(name, feat, hidden, n_out, torch.float32 if dt == F32 else torch.bfloat16) == bool(want)


# ------------------------------------------------------------------------------------------------------------ the wrapper
def cpu_block(relabel=True):
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return gnc.Block(i32([0, 2, 2]), i32([1, 0]), i32([5, 7]) if relabel else None, None, 2, 2 if relabel else 10, 2)


X, W1, W2 = torch.zeros(10, 4), torch.zeros(8, 5), torch.zeros(5, 3)
OK = dict(x=X, w1=W1, w2=W2)
WRAPPER = [
    ("unknown reduce", dict(OK, reduce="min"), ValueError, "reduce"),
    ("unknown combine", dict(OK, combine="mul"), ValueError, "combine"),
    ("out_dtype float16", dict(OK, out_dtype=torch.float16), TypeError, "out_dtype"),
    ("x float16", dict(x=X.half(), w1=W1.half(), w2=W2.half()), TypeError, "x must be"),
    ("x 1-D", dict(OK, x=torch.zeros(10)), ValueError, "2-D"),
    ("a gathered x with too few rows", dict(OK, x=torch.zeros(1, 4), gathered=True), ValueError, "rows"),
    ("w1 no tensor", dict(OK, w1=np.zeros((8, 5), np.float32)), TypeError, "w1"),
    ("w2 of another dtype", dict(OK, w2=W2.bfloat16()), TypeError, "w2"),
    ("w1 with F rows, not 2 F", dict(OK, w1=torch.zeros(4, 5)), ValueError, "w1"),
    ("w2 that does not follow w1", dict(OK, w2=torch.zeros(4, 3)), ValueError, "w2"),
    ("b1 bfloat16", dict(OK, b1=torch.zeros(5, dtype=torch.bfloat16)), TypeError, "b1"),
    ("b1 of the length of b2", dict(OK, b1=torch.zeros(3)), ValueError, "b1"),
    ("b2 of the length of b1", dict(OK, b2=torch.zeros(5)), ValueError, "b2"),
    ("out of the wrong shape", dict(OK, out=torch.zeros(2, 5)), ValueError, "out must be"),
    ("out against out_dtype", dict(x=X.bfloat16(), w1=W1.bfloat16(), w2=W2.bfloat16(), out=torch.zeros(2, 3), out_dtype=torch.bfloat16),
     TypeError, "out_dtype"),
    ("a bfloat16 out of float32 operands", dict(OK, out_dtype=torch.bfloat16), TypeError, "out_dtype"),
    ("fused=True outside the range", dict(OK, w1=torch.zeros(8, 300), w2=torch.zeros(300, 3), fused=True), ValueError, "fused=True"),
    ("x on the host", OK, ValueError, "device tensor"),
    ("x on the host, composition", dict(OK, fused=False), ValueError, "device tensor"),
]


@pytest.mark.parametrize("what,kw,exc,word", WRAPPER, ids=[w[0] for w in WRAPPER])
def test_wrapper_refusals_are_raised_before_device_work(what, kw, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        cpu_block().edgeconv(**kw)
    with pytest.raises(exc, match=re.escape(word)):
        gnc.block_edgeconv_run(cpu_block(), **kw)
