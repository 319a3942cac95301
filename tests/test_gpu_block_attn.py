"""GPU: Block.attend / gnnagg_block_attn_run (include/gnnagg.h section F, "Block attention") -- GATv2 and dot-product attention on the
synthetic block of tests/block_run_ref.py in one launch, read through src_nodes and eid.  The yardsticks are the suite's own: the float64
judges and bounds of the handle's calls (every row), and Aggregator_GAT(blk.ptr, blk.idx).run_dot / run_v2 on the gathered operands bit
for bit (rows of at most 128 edges: the longer ones are folded in segments by the handle and walked by one lane group here)."""
import functools
import math

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc

import block_run_ref as br
from test_attn_bias_host import dot_attn_bias_ref, gatv2_bias_ref
from test_attn_edge_host import dot_attn_edge_ref, gatv2_edge_ref
from test_dot_attn_host import dot_attn_bound, dot_attn_ref
from test_gatv2_host import gatv2_bound, gatv2_ref, worst_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, B16 = torch.float32, torch.bfloat16
SLOPE = 0.2
SB = br.synthetic_block()
N, PTR, IDX, SRC, EID = SB["num_dst"], SB["ptr"], SB["idx"], SB["src_nodes"], SB["eid"]
DEG = br.degrees(PTR)
SHORT = torch.from_numpy(DEG <= 128)          # the rows that owe the handle's bits
EMPTY = int(np.flatnonzero(DEG == 0)[0])
MASKED = int(np.flatnonzero(DEG == 7)[0])     # the row a bias masks whole
KINDS = ("dot", "gatv2")
SHAPES = [(1, 3), (1, 8), (4, 8), (8, 16), (1, 128), (4, 128), (1, 100), (1, 602)]


def dev(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dt)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def tblock(src=True, eid=True, n=N):
    """the first n rows of the synthetic block on the device: relabelled (src_nodes) or, src=False, with ids into the gathered rows"""
    ne = int(PTR[n])
    return gnc.Block(dev(PTR[:n + 1], torch.int32), dev(IDX[:ne], torch.int32), dev(SRC, torch.int32) if src else None,
                     dev(EID[:ne], torch.int32) if eid else None, n, SB["num_src"], ne)


@functools.lru_cache(maxsize=None)
def operands(H, D):
    """host float32 arrays a bfloat16 holds exactly, one row per row of the FULL graph: q, k, v [NUM_X, F] and a [H, D]"""
    rng = np.random.default_rng(100 * H + D)
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(B16).float().numpy()
    return dict(q=rnd(br.NUM_X, H * D), k=rnd(br.NUM_X, H * D), v=rnd(br.NUM_X, H * D), a=rnd(H, D) / np.float32(2 ** round(math.log2(D) / 2)))


def attend(blk, kind, ops, H, xdt=F32, out=None, **kw):
    """Block.attend on host operand arrays (q / k / v / a), y pre-filled so that an unwritten element shows"""
    if out is None:
        out = torch.full((blk.num_dst, ops["q"].shape[1]), 7.0, device=DEV, dtype=kw.pop("out_dtype", None) or F32)
    q, k = dev(ops["q"], xdt), dev(ops["k"], xdt)
    if kind == "dot":
        return blk.attend(q, k, dev(ops["v"], xdt), heads=H, out=out, **kw)
    return blk.attend(q, k, kind="gatv2", a=dev(ops["a"]), heads=H, slope=SLOPE, out=out, **kw)


def handle(kind, g, H, xdt=F32, **kw):
    """the yardstick: a handle over the block's CSR on the gathered operands"""
    agg = gnc.Aggregator_GAT(dev(PTR, torch.int32), dev(IDX, torch.int32))
    y = torch.full((N, g["q"].shape[1]), 7.0, device=DEV)
    if kind == "dot":
        agg.run_dot(dev(g["q"], xdt), dev(g["k"], xdt), dev(g["v"], xdt), y, heads=H, **kw)
    else:
        agg.run_v2(dev(g["k"], xdt), dev(g["q"], xdt), dev(g["a"]), y, heads=H, slope=SLOPE, **kw)
    torch.cuda.synchronize()
    agg.close()
    return y


def judge(kind, g, H, bias=None, ef=None):
    """(float64 y, bound) of the suite's judge for these operands: plain, with a bias, or with edge rows (and a bias)"""
    D = g["q"].shape[1] // H
    sc = 1.0 / math.sqrt(D)
    with np.errstate(all="ignore"):
        if ef is not None:
            y, L, S = (dot_attn_edge_ref(PTR, IDX, g["q"], g["k"], g["v"], ef, H, sc, bias) if kind == "dot" else
                       gatv2_edge_ref(PTR, IDX, g["k"], g["q"], g["a"], ef, H, SLOPE, bias))
        elif bias is not None:
            y, L, S = (dot_attn_bias_ref(PTR, IDX, g["q"], g["k"], g["v"], H, sc, bias) if kind == "dot" else
                       gatv2_bias_ref(PTR, IDX, g["k"], g["q"], g["a"], H, SLOPE, bias))
        else:
            y, L, S = (dot_attn_ref(PTR, IDX, g["q"], g["k"], g["v"], H, sc) if kind == "dot" else gatv2_ref(PTR, IDX, g["k"], g["q"], g["a"], H, SLOPE))
    return y, (dot_attn_bound if kind == "dot" else gatv2_bound)(L, S, H)


def gathered(ops):
    return dict(q=ops["q"][SRC], k=ops["k"][SRC], v=ops["v"][SRC], a=ops["a"])


def inside(y, ref, bound, what):
    """every finite row of the judge inside its bound (ratio printed), NaN exactly where the judge has it (a row masked whole)"""
    y = y.float().cpu().numpy()
    fin = ~np.isnan(ref)
    assert np.array_equal(np.isnan(y), ~fin), what
    ratio = worst_ratio(y[fin], ref[fin], bound[fin])
    print("%s: worst |y - ref| / bound = %.4f" % (what, ratio))
    assert ratio <= 1.0, what


# --------------------------------------------------------------------------------------- 1. the float64 judge and the handle, every geometry
@pytest.mark.parametrize("H,D", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_against_the_judge_and_the_handle(kind, H, D):
    ops = operands(H, D)
    g = gathered(ops)
    ref, bound = judge(kind, g, H)
    blk = tblock()
    for xdt in (F32, B16):
        what = "%s H=%d D=%d %s" % (kind, H, D, xdt)
        y = attend(blk, kind, ops, H, xdt)
        inside(y, ref, bound, what)
        assert same_bits(y[SHORT], handle(kind, g, H, xdt)[SHORT]), what + ": rows of <= 128 edges differ from the handle"
        assert not bits(y[EMPTY]).any(), what + ": the row without edges is not +0"
        y16 = attend(blk, kind, ops, H, xdt, out_dtype=B16)
        assert same_bits(y16, y.to(B16)), what + ": a bf16 y is not one rounding of the fp32 y"
        assert same_bits(attend(blk, kind, g, H, xdt, gathered=True), y), what + ": gathered=True differs from the mapped call"
        assert same_bits(attend(tblock(src=False), kind, g, H, xdt), y), what + ": a block of direct ids differs from the mapped call"


# --------------------------------------------------------------------------------------- 2. per-edge operands through eid
@pytest.mark.parametrize("H,D", [(4, 32), (2, 3)])     # segmented (16- / 32-lane groups, 4 / 8 lanes per head); general
@pytest.mark.parametrize("kind", KINDS)
def test_bias_and_edge_rows_through_eid(kind, H, D):
    ops = operands(H, D)
    g = gathered(ops)
    blk = tblock()
    rng = np.random.default_rng(5 + H)
    rnd = lambda *s: torch.from_numpy(2.0 * rng.standard_normal(s).astype(np.float32)).to(B16).float().numpy()
    ef_full = rnd(br.NUM_E_FULL, H * D) / np.float32(2)
    biases = {"[E]": rnd(br.NUM_E_FULL), "[E, heads]": rnd(br.NUM_E_FULL, H)}
    for b in biases.values():                                    # masks: scattered edges and one row whole
        b[rng.choice(br.NUM_E_FULL, br.NUM_E_FULL // 10, replace=False)] = -np.inf
        b[EID[PTR[MASKED]:PTR[MASKED + 1]]] = -np.inf
    for xdt in (F32, B16):
        cases = [(name, b, None) for name, b in biases.items()] + [("edge", None, ef_full), ("edge + [E]", biases["[E]"], ef_full),
                                                                   ("edge + [E, heads]", biases["[E, heads]"], ef_full)]
        for name, b_full, e_full in cases:
            what = "%s H=%d D=%d %s %s" % (kind, H, D, xdt, name)
            full, per_edge, href = {}, {}, {}
            if b_full is not None:
                full.update(bias=dev(b_full), bias_full=True)
                per_edge.update(bias=dev(b_full[EID]))
                href.update(bias=dev(b_full[EID]))
            if e_full is not None:
                full.update(edge=dev(e_full, xdt), edge_full=True)
                per_edge.update(edge=dev(e_full[EID], xdt))
                href.update(edge=dev(e_full[EID], xdt))
            y = attend(blk, kind, ops, H, xdt, **per_edge)
            assert same_bits(attend(blk, kind, ops, H, xdt, **full), y), what + ": through eid differs from the per-block-edge call"
            assert same_bits(y[SHORT], handle(kind, g, H, xdt, **href)[SHORT]), what + ": rows of <= 128 edges differ from the handle"
            ref, bound = judge(kind, g, H, None if b_full is None else b_full[EID], None if e_full is None else e_full[EID])
            inside(y, ref, bound, what)


# --------------------------------------------------------------------------------------- 3. addressing
@pytest.mark.parametrize("kind", KINDS)
def test_column_views_and_unaligned_operands_keep_the_bits(kind):
    H, D = 4, 8
    F = H * D
    ops = operands(H, D)
    blk = tblock()
    for xdt in (F32, B16):
        y = attend(blk, kind, ops, H, xdt)
        qkv = dev(np.concatenate([ops["q"], ops["k"], ops["v"]], 1), xdt)          # column views of one [n, 3F] tensor
        q, k, v = qkv[:, :F], qkv[:, F:2 * F], qkv[:, 2 * F:]

        def off1(t):                                                             # the same values one element past an aligned base
            flat = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
            flat[1:] = t.reshape(-1)
            return flat[1:].view(t.shape)
        for what, (q_, k_, v_), out in (("column views", (q, k, v), torch.full_like(y, 7.0)),
                                        ("offset by one element", [off1(t.contiguous()) for t in (q, k, v)], off1(torch.full_like(y, 7.0)))):
            if kind == "dot":
                got = blk.attend(q_, k_, v_, heads=H, out=out)
            else:
                got = blk.attend(q_, k_, kind="gatv2", a=dev(ops["a"]), heads=H, slope=SLOPE, out=out)
            assert same_bits(got, y), "%s %s: %s" % (kind, xdt, what)


@pytest.mark.parametrize("H,D,rows_per_workgroup", [(4, 8, 8), (1, 3, 4)])     # 8-lane groups; 64-lane groups
@pytest.mark.parametrize("kind", KINDS)
def test_num_dst_around_a_workgroup(kind, H, D, rows_per_workgroup):
    ops = operands(H, D)
    y = attend(tblock(), kind, ops, H)
    for n in (0, 1, rows_per_workgroup - 1, rows_per_workgroup + 1):
        buf = torch.full((n + 1, H * D), 7.0, device=DEV)
        got = attend(tblock(n=n), kind, ops, H, out=buf[:n])
        assert same_bits(got, y[:n]) and bool((buf[n] == 7.0).all()), "%s H=%d D=%d num_dst=%d" % (kind, H, D, n)


# --------------------------------------------------------------------------------------- 4. one capture
def test_a_captured_call_replays_the_eager_bits():
    H, D = 4, 8
    ops = operands(H, D)
    blk = tblock()
    q, k, v = (dev(ops[n], B16) for n in "qkv")
    bias = dev(np.random.default_rng(3).standard_normal(br.NUM_E_FULL).astype(np.float32))
    eager = blk.attend(q, k, v, heads=H, bias=bias, bias_full=True, out_dtype=F32)
    out = torch.empty_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        blk.attend(q, k, v, heads=H, bias=bias, bias_full=True, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        blk.attend(q, k, v, heads=H, bias=bias, bias_full=True, out=out)
    for _ in range(3):
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, eager)
