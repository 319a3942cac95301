"""CPU: gnnagg_block_gcn_run (include/gnnagg.h section F, "Block aggregation") without a device -- the surface (header, export, ctypes
signature, KFILES), every refusal the contract lists (decided before any HIP call, so they answer here), the wrapper's TypeError /
ValueError cases, and the numpy restatement against a 3-row example worked by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

import block_run_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn_computing_amd", "csrc")
NAME = "gnnagg_block_gcn_run"
VP, CI, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
ARGS = [VP, VP, CI, VP, VP, VP, VP, CI, LL, VP, CI, VP, CI, CI, CI, VP]


# ------------------------------------------------------------------------------------------------------------ the surface
def test_declared_exported_typed_and_built():
    text = open(os.path.join(ROOT, "include", "gnnagg.h")).read()
    assert re.search(r"^int gnnagg_block_gcn_run\(const int \*d_blk_ptr, const int \*d_blk_idx, int num_dst, const int \*d_src_nodes, "
                     r"const float \*d_val,\s+const int \*d_eid, const void \*d_x, int x_dtype, long long x_pitch, void \*d_y, int y_dtype, "
                     r"void \*d_x_dst,\s+int feat, int reduce, int flags, void \*hip_stream\);", text, re.M)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert NAME in {l.split()[-1] for l in out.splitlines() if " T " in l}
    res, got = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and got == ARGS
    assert getattr(gnc.lib(), NAME).argtypes == ARGS
    kfiles = re.search(r"^KFILES := (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "agg_block" in kfiles and os.path.exists(os.path.join(CSRC, "agg_block.hip"))
    assert callable(gnc.block_gcn_run) and callable(gnc.Block.aggregate)


def test_block_fields_are_unchanged():
    assert gnc.Block._fields == ("ptr", "idx", "src_nodes", "eid", "num_dst", "num_src", "num_edges")
    assert callable(gnc.Block.gcn) and callable(gnc.Block.gat)


def test_the_kernel_file_uses_the_shared_dispatch_and_adds_no_label():
    text = open(os.path.join(CSRC, "agg_block.hip")).read()
    assert "DISPATCH_GEOM(" in text and "DISPATCH_GEOM_16BIT(" in text
    assert not re.search(r"\bcase \d+:", text)
    assert "pick_geometry(" in text and "typed_geometry(" in text
    for word in ("atomic", "__shared__"):
        assert word not in re.sub(r"//[^\n]*", "", text), word


# ------------------------------------------------------------------------------------------------------------ the refusals
# a call that would be valid on a device: fake non-null addresses (never dereferenced: a refusal comes before any HIP call)
GOOD = dict(ptr=0x1000, idx=0x2000, num_dst=4, src=0x3000, val=0x4000, eid=0x5000, x=0x6000, x_dtype=_lib.DTYPE_F32, x_pitch=16, y=0x7000,
            y_dtype=_lib.DTYPE_BF16, x_dst=0x8000, feat=16, reduce=_lib.REDUCE_MEAN, flags=_lib.FLAG_RELU, stream=None)
ORDER = ("ptr", "idx", "num_dst", "src", "val", "eid", "x", "x_dtype", "x_pitch", "y", "y_dtype", "x_dst", "feat", "reduce", "flags", "stream")

REFUSALS = [
    ("null blk_ptr", dict(ptr=None), "d_blk_ptr"),
    ("null x", dict(x=None), "d_x"),
    ("null y", dict(y=None), "d_y"),
    ("negative num_dst", dict(num_dst=-1), "num_dst"),
    ("feat 0", dict(feat=0), "feat"),
    ("negative feat", dict(feat=-3), "feat"),
    ("pitch below feat", dict(x_pitch=15), "x_pitch"),
    ("unknown x dtype", dict(x_dtype=2), "x_dtype"),
    ("unknown y dtype", dict(y_dtype=-1), "y_dtype"),
    ("unknown reduce", dict(reduce=3), "reduce"),
    ("the accumulate flag", dict(flags=_lib.FLAG_ACCUMULATE), "flags"),
    ("an unknown flag beside relu", dict(flags=_lib.FLAG_RELU | 4), "flags"),
    ("eid without val", dict(val=None), "d_eid"),
    ("x_dst without src_nodes", dict(src=None), "d_x_dst"),
]


def call(**over):
    a = dict(GOOD, **over)
    return gnc.lib().gnnagg_block_gcn_run(*[a[k] for k in ORDER])


@pytest.mark.parametrize("what,over,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_device_call(what, over, word):
    assert call(**over) == _lib.ERR_ARG
    msg = gnc.lib().gnnagg_last_error().decode()
    assert msg.startswith(NAME + ": ") and word in msg, msg


def test_null_pointers_are_fine_where_nothing_is_read():
    # num_dst = 0 launches nothing, whatever the pointers are -- and still refuses what is wrong whatever num_dst is
    assert call(num_dst=0, ptr=None, idx=None, x=None, y=None, x_dst=None, src=None, val=None, eid=None) == _lib.OK
    assert call(num_dst=0, feat=0) == _lib.ERR_ARG
    assert call(num_dst=0, val=None) == _lib.ERR_ARG


# ------------------------------------------------------------------------------------------------------------ the wrapper
def cpu_block(eid=False, relabel=True):
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return gnc.Block(i32([0, 2, 2]), i32([1, 0]), i32([5, 7]) if relabel else None, i32([3, 9]) if eid else None, 2, 2 if relabel else 10, 2)


X = torch.zeros(10, 4)
WRAPPER = [
    ("unknown reduce", cpu_block(), dict(x=X, reduce="prod"), ValueError, "reduce"),
    ("val_full without eid", cpu_block(), dict(x=X, val=torch.zeros(20), val_full=True), ValueError, "eid"),
    ("val_full without val", cpu_block(eid=True), dict(x=X, val_full=True), ValueError, "val"),
    ("return_dst of a gathered x", cpu_block(), dict(x=X, gathered=True, return_dst=True), ValueError, "return_dst"),
    ("return_dst of a global-id block", cpu_block(relabel=False), dict(x=X, return_dst=True), ValueError, "return_dst"),
    ("out_dtype float16", cpu_block(), dict(x=X, out_dtype=torch.float16), TypeError, "out_dtype"),
    ("x no tensor", cpu_block(), dict(x=np.zeros((10, 4), np.float32)), TypeError, "x must be"),
    ("x float16", cpu_block(), dict(x=X.half()), TypeError, "x must be"),
    ("x int32", cpu_block(), dict(x=X.int()), TypeError, "x must be"),
    ("x 1-D", cpu_block(), dict(x=torch.zeros(10)), ValueError, "2-D"),
    ("x without columns", cpu_block(), dict(x=torch.zeros(10, 0)), ValueError, "F >= 1"),
    ("a gathered x with too few rows", cpu_block(), dict(x=torch.zeros(1, 4), gathered=True), ValueError, "rows"),
    ("val float64", cpu_block(), dict(x=X, val=torch.zeros(2, dtype=torch.float64)), TypeError, "val"),
    ("val of the wrong length", cpu_block(), dict(x=X, val=torch.zeros(3)), ValueError, "val"),
    ("val 2-D", cpu_block(), dict(x=X, val=torch.zeros(2, 1)), ValueError, "val"),
    ("out float16", cpu_block(), dict(x=X, out=torch.zeros(2, 4, dtype=torch.float16)), TypeError, "out"),
    ("out against out_dtype", cpu_block(), dict(x=X, out=torch.zeros(2, 4), out_dtype=torch.bfloat16), TypeError, "out_dtype"),
    ("out of the wrong shape", cpu_block(), dict(x=X, out=torch.zeros(3, 4)), ValueError, "out must be"),
    ("return_dst of another dtype", cpu_block(), dict(x=X, return_dst=torch.zeros(2, 4, dtype=torch.bfloat16)), TypeError, "return_dst"),
    ("return_dst of the wrong shape", cpu_block(), dict(x=X, return_dst=torch.zeros(2, 5)), ValueError, "return_dst"),
    ("x on the host", cpu_block(), dict(x=X), ValueError, "device tensor"),
]


@pytest.mark.parametrize("what,blk,kw,exc,word", WRAPPER, ids=[w[0] for w in WRAPPER])
def test_wrapper_refusals_are_raised_before_device_work(what, blk, kw, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        blk.aggregate(**kw)
    with pytest.raises(exc, match=re.escape(word)):
        gnc.block_gcn_run(blk, **kw)


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_against_a_three_row_example_worked_by_hand():
    # x has 5 rows; the block's 3 source rows are x[4], x[0], x[2] (src_nodes); row 0 holds sources 1, 2; row 1 none; row 2 holds 0, 0, 1
    x = np.array([[1, -2], [100, 100], [3, 4], [100, 100], [-5, 6]], np.float32)
    src = np.array([4, 0, 2], np.int32)
    ptr, idx = np.array([0, 2, 2, 5], np.int32), np.array([1, 2, 0, 0, 1], np.int32)
    # row 0: x[0] + x[2] = (4, 2); row 2: x[4] + x[4] + x[0] = (-9, 10)
    assert np.array_equal(br.chain32(ptr, idx, x, "sum", src_nodes=src), [[4, 2], [0, 0], [-9, 10]])
    assert np.array_equal(br.chain32(ptr, idx, x, "mean", src_nodes=src), [[2, 1], [0, 0], [-3, np.float32(10) / np.float32(3)]])
    assert np.array_equal(br.chain32(ptr, idx, x, "max", src_nodes=src), [[3, 4], [0, 0], [1, 6]])
    assert np.array_equal(br.chain32(ptr, idx, x, "sum", src_nodes=src, relu=True), [[4, 2], [0, 0], [0, 10]])
    # the same through an already gathered x
    assert np.array_equal(br.chain32(ptr, idx, x[src], "sum"), [[4, 2], [0, 0], [-9, 10]])
    # weights: per edge of the block, or of a full CSR of 8 edges through eid
    val = np.array([0.5, 2, -1, 0.25, 4], np.float32)
    full, eid = np.zeros(8, np.float32), np.array([6, 7, 0, 2, 3], np.int32)
    full[eid] = val
    # row 0: .5 (1, -2) + 2 (3, 4) = (6.5, 7); row 2: -(-5, 6) + .25 (-5, 6) + 4 (1, -2) = (7.75, -12.5)
    want = [[6.5, 7], [0, 0], [7.75, -12.5]]
    assert np.array_equal(br.chain32(ptr, idx, x, "sum", val=val, src_nodes=src), want)
    assert np.array_equal(br.chain32(ptr, idx, x, "sum", val=full, src_nodes=src, eid=eid), want)
    # max over w * x: row 0: max(.5, 6), max(-1, 8); row 2: max(5, -1.25, 4), max(-6, 1.5, -8)
    assert np.array_equal(br.chain32(ptr, idx, x, "max", val=val, src_nodes=src), [[6, 8], [0, 0], [5, 1.5]])
    s, scale = br.sum64(ptr, idx, x, val=full, src_nodes=src, eid=eid)
    assert np.array_equal(s, want) and np.array_equal(scale, [[6.5, 9], [0, 0], [10.25, 15.5]])
    # a NaN stays a NaN under ReLU, -Inf becomes 0
    xn = np.array([[np.nan, -np.inf]], np.float32)
    assert np.array_equal(br.chain32(np.array([0, 1]), np.array([0]), xn, "sum", relu=True), [[np.nan, 0]], equal_nan=True)


def test_the_synthetic_block_holds_what_it_promises():
    b = br.synthetic_block()
    assert list(br.degrees(b["ptr"])) == br.DEGREES and b["num_edges"] == sum(br.DEGREES) == len(b["idx"]) == len(b["eid"])
    for g in (8, 16, 32, 64):
        assert {g - 1, g, g + 1} <= set(br.DEGREES)
    assert 0 in br.DEGREES and max(br.DEGREES) > 4 * 64
    assert b["idx"].min() >= 0 and b["idx"].max() < br.NUM_SRC and len(np.unique(b["idx"])) < len(b["idx"])   # repeats
    assert len(b["src_nodes"]) == br.NUM_SRC == len(np.unique(b["src_nodes"])) and b["src_nodes"].max() < br.NUM_X
    assert not np.array_equal(b["src_nodes"], np.arange(br.NUM_SRC))
    assert len(np.unique(b["eid"])) == len(b["eid"]) and b["eid"].max() < br.NUM_E_FULL and b["num_dst"] <= br.NUM_SRC
