"""Host: the inputs, judges and expectations of tests/test_gpu_attn_nonfinite.py -- non-finite scores and features on the two online-softmax
attention calls (gnnagg_gatv2_run, gnnagg_dot_attn_run) -- pinned without a GPU.

The judges stay the plain two-pass float64 formulas (gatv2_ref of tests/test_gatv2_host.py, dot_attn_ref of tests/test_dot_attn_host.py):
numpy propagates IEEE classes through them, so the judge of a non-finite result is its CLASS MAP (classes / assert_same_classes of
tests/test_nonfinite_host.py).  This file adds

  * masked_case: operands in which chosen edges score -Inf in ONE head (a reserved set of source ids >= V, named by the masked edges only);
  * the bound of a masked case, taken from the reference on the graph with the masked edges DELETED (L over the full graph is Inf), and the
    proof that both references are one judge (equal to float64 rounding, 1e-7 of the bound, NaN = NaN, apart from GATv2's NaN column);
  * an fp32 emulation of the kernels' online recurrence for one (row, head, column): batches of 2 and 4 edges, the chunks of a segment
    folded in ascending order, the segments merged in ascending order -- in the fixed form and, behind a flag, in the form before the fix,
    which is the regression's witness on the CPU: NaN where the first full batch, or a whole chunk, is masked;
  * gatv2_geometry in Python and the proof that SHAPES reaches every instantiation of attn_launch_typed (both kernels);
  * the condition that keeps the class map independent of the kernel's order: the finite float64 scores of a (row, head) spread by less than
    60, so no fp32 weight or rescale factor underflows to 0 where float64's does not (exp(-60) = 8.8e-27)."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from test_dot_attn_host import dot_attn_bound, dot_attn_ref
from test_gatv2_host import gatv2_bound, gatv2_ref
from test_gpu_gatv2 import threshold_graph
from test_nonfinite_host import classes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn_computing_amd", "csrc")
THRESHOLDS = gnc.Aggregator_GAT.GATV2_THRESHOLDS
BATCH, LONG, SEG = THRESHOLDS[0], THRESHOLDS[-2], THRESHOLDS[-1]
NINF = -np.inf
SPREAD = 60.0
SLOPE = 0.2

# (heads, D): every instantiation of the shared launcher (both kernels), fp32 and bf16 (test_the_shapes_reach_every_instantiation)
SHAPES = [(1, 8), (4, 16), (8, 16), (8, 32), (4, 128), (8, 128), (4, 3), (1, 100), (1, 200), (2, 301), (1, 1000)]

# which edges of every row with edges are masked
PATTERNS = [("first", 1), ("first", 2), ("first", 3), ("first", 4), ("first", 5), ("first", 8), "all_but_last", "last", "every_second",
            "half_segment", ("segment", "first"), ("segment", "middle"), ("segment", "last"), "all"]


def pattern_id(p):
    return p if isinstance(p, str) else "%s_%s" % p


# ------------------------------------------------------------------------------------------------ the lane geometry, restated
def geometry(F, heads, esize):
    """gatv2_geometry of csrc/gatv2_shared.cuh: (vec, group, fragments per lane, lanes per head, segmented)"""
    D, vec = F // heads, 16 // esize
    if D % vec == 0:
        lph = D // vec
        if lph & (lph - 1) == 0 and lph <= 64:
            lanes = F // vec
            group = 8
            while group < 64 and group < lanes:
                group <<= 1
            nf = -(-lanes // group)
            return dict(vec=vec, group=group, nf=1 if nf <= 1 else 2 if nf <= 2 else 4, lph=lph, segred=True)
    nf = (F + 63) // 64
    return dict(vec=1, group=64, nf=next(n for n in (1, 2, 4, 10, 16) if nf <= n), lph=0, segred=False)


def groups_per_block(group):
    """block_of<GROUP>() / GROUP: the lane groups that share a segment"""
    return min(group * 8, 256) // group


def dot_batch(nf):
    """dot_batch<NF>() of csrc/agg_dot.hip"""
    return BATCH // 2 if nf >= 2 else BATCH


def chunk_edges(n, gpb):
    """edges per lane group of a segment of n edges (k_gatv2 / k_dot_attn: the ceiling, rounded up to whole batches of kGatv2Batch)"""
    return -(-(-(-n // gpb)) // BATCH) * BATCH


def leading_half(n):
    """edges at the head of a segment of n edges that are whole leading chunks with 8 lane groups AND with 4 (about half of it)"""
    return max(4 * chunk_edges(n, 8), 2 * chunk_edges(n, 4))


def test_the_shapes_reach_every_instantiation():
    # the one switch pair (gatv2_shared.cuh: attn_launch_typed) ...
    text = open(os.path.join(CSRC, "gatv2_shared.cuh")).read()
    body = text[text.index("static int attn_launch_typed"):]
    body = body[:body.index("\n}\n")]
    inst = re.findall(r"(if constexpr \(VEC == 4\) )?return attn_launch_inst<K, (VEC|1), (\d+), (\d+), TX, (true|false)>", body)
    assert len(inst) == 11
    insts = {(int(g), int(nf), seg == "true", bool(only4)) for only4, _, g, nf, seg in inst}
    # ... through which both kernels are launched, in both element types: neither file has instantiations of its own
    for name, functor in (("agg_gatv2.hip", "Gatv2Kernel"), ("agg_dot.hip", "DotKernel")):
        text = open(os.path.join(CSRC, name)).read()
        assert len(re.findall(r"return attn_launch_typed<%s, (?:8, __bf16|4, float)>\(a, g, stream, no_inst\);" % functor, text)) == 2
        assert "attn_launch_inst<" not in text and not re.search(r"\bswitch\s*\(", text)
    seg = {(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4)}
    assert {(g, nf) for g, nf, s, _ in insts if s} == seg and {nf for g, nf, s, _ in insts if not s} == {1, 2, 4, 10, 16}
    assert {(g, nf) for g, nf, s, only4 in insts if only4} == {(64, 4)}     # fp32 only: bf16 has at most 128 16-byte lanes
    for esize in (4, 2):
        got = set()
        for H, D in SHAPES:
            g = geometry(H * D, H, esize)
            got.add((g["group"], g["nf"], g["segred"]))
        expect = {(g, nf, s) for g, nf, s, only4 in insts if not (only4 and esize == 2)}
        assert got == expect, (esize, sorted(expect - got))
    # both batches of the dot kernel, and both numbers of lane groups, occur
    assert {dot_batch(geometry(H * D, H, e)["nf"]) for H, D in SHAPES for e in (4, 2)} == {2, 4}
    assert {groups_per_block(geometry(H * D, H, e)["group"]) for H, D in SHAPES for e in (4, 2)} == {4, 8}
    # the restatement against what the header of the kernel file says
    assert geometry(8, 1, 4) == dict(vec=4, group=8, nf=1, lph=2, segred=True) and geometry(8, 1, 2)["lph"] == 1
    assert geometry(1024, 8, 4)["nf"] == 4 and geometry(1024, 8, 2)["nf"] == 2 and not geometry(100, 1, 4)["segred"]
    assert geometry(1000, 1, 2) == dict(vec=1, group=64, nf=16, lph=0, segred=False)


# ------------------------------------------------------------------------------------------------ inputs
def bf16_exact(a):
    """float32 numpy values that a bf16 tensor holds exactly: one set of values serves the fp32 and the bf16 runs and the judge"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def randn(shape, seed):
    return bf16_exact(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32))


def mask_edges(ptr, pattern):
    """bool [E]: the edges `pattern` masks"""
    ptr = np.asarray(ptr, np.int64)
    deg = np.diff(ptr)
    mask = np.zeros(int(ptr[-1]), bool)
    kind, arg = (pattern, None) if isinstance(pattern, str) else pattern
    for r in np.flatnonzero(deg > 0):
        b, n = int(ptr[r]), int(deg[r])
        if kind == "first":
            mask[b:b + min(arg, n)] = True
        elif kind == "all_but_last":
            mask[b:b + n - 1] = True
        elif kind == "last":
            mask[b + n - 1] = True
        elif kind == "every_second":
            mask[b:b + n:2] = True
        elif kind == "half_segment":
            if n > LONG:
                mask[b:b + leading_half(min(n, SEG))] = True
        elif kind == "segment":
            nseg = -(-n // SEG)
            s = {"first": 0, "middle": nseg // 2 if nseg >= 3 else None, "last": nseg - 1}[arg]
            if n > SEG and s is not None:
                mask[b + s * SEG:min(b + (s + 1) * SEG, b + n)] = True
        else:
            assert kind == "all"
            mask[b:b + n] = True
    return mask


def delete_edges(ptr, idx, mask):
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    keep = ~mask
    ptr_d = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=len(ptr) - 1))]).astype(np.int32)
    return ptr_d, np.ascontiguousarray(idx[keep])


N_RESERVED = 8


def reserve_sources(idx, n_src, n=N_RESERVED):
    """idx with no edge naming the last n source ids (such edges name the id n below), and those ids"""
    idx = np.array(idx, dtype=np.int32, copy=True)
    idx[idx >= n_src - n] -= n
    return idx, np.arange(n_src - n, n_src)


JUDGE_BLOCK = 1024   # edges per block of the float64 judges: temporaries that stay in cache


@functools.lru_cache(maxsize=64)
def _attn_operands(call, V, n_src, H, D, h, seed):
    F, c = H * D, h * D
    if call == "dot":
        q, k, v = randn((V, F), seed), randn((n_src, F), seed + 1), randn((n_src, F), seed + 2)
        q[:, c] = bf16_exact(np.abs(q[:, c]) + 0.5)
        return dict(q=q, k=k, v=v)
    xs, xd = randn((n_src, F), seed), randn((V, F), seed + 1)
    a = (np.random.default_rng(seed + 2).standard_normal((H, D), dtype=np.float32) / np.float32(math.sqrt(D))).astype(np.float32)
    a[h, 0] = abs(a[h, 0]) + np.float32(0.1)
    a[a == 0] = np.float32(0.25)       # (group c: an Inf column times a zero would be a NaN of the generator's making)
    return dict(xs=xs, xd=xd, a=a)


def attn_operands(call, V, n_src, H, D, h, seed):
    """clean operands of one call with the masking column of head h made positive: the score of a source that is -Inf there is -Inf.
    dot: (q, k, v), q[:, hD] = |q| + 0.5, default scale.  v2: (xs, xd, a), a = randn / sqrt(D) with a[h, 0] > 0, slope 0.2.
    The arrays are shared between calls with the same arguments: copy before writing."""
    ops = _attn_operands(call, V, n_src, H, D, h, seed)
    for x in ops.values():
        x.setflags(write=False)
    return dict(ops)


SCORED = {"dot": "k", "v2": "xs"}     # the gathered operand the score is formed from
ROWWISE = {"dot": "q", "v2": "xd"}    # the operand read once per row


def masked_case(call, ptr, idx, n_src, H, D, h, mask, seed=0):
    """The operands in which the edges `mask` selects score -Inf in head h only: their idx is redirected to a reserved set of source ids
    (>= V, named by no other edge) whose scored operand is -Inf at column hD.  Returns (idx, clean operands, masked operands)."""
    V = len(ptr) - 1
    idx2, reserved = reserve_sources(idx, n_src)
    assert reserved.min() >= V
    idx2[mask] = reserved[np.arange(int(mask.sum())) % len(reserved)]
    clean = attn_operands(call, V, n_src, H, D, h, seed)
    masked = dict(clean)
    masked[SCORED[call]] = clean[SCORED[call]].copy()
    masked[SCORED[call]][reserved, h * D] = NINF
    return idx2, clean, masked


def default_scale(D):
    return np.float32(1.0 / math.sqrt(D))


def head_ref(call, ptr, idx, ops, H, h):
    """the float64 judge on head h's columns alone (heads are independent): (y [V, D], L [V, 1], S [V, D])"""
    D = ops[SCORED[call]].shape[1] // H
    sl = slice(h * D, (h + 1) * D)
    with np.errstate(all="ignore"):
        if call == "dot":
            return dot_attn_ref(ptr, idx, ops["q"][:, sl], ops["k"][:, sl], ops["v"][:, sl], 1, default_scale(D), block_edges=JUDGE_BLOCK)
        return gatv2_ref(ptr, idx, ops["xs"][:, sl], ops["xd"][:, sl], ops["a"][h:h + 1], 1, SLOPE, block_edges=JUDGE_BLOCK)


def full_ref(call, ptr, idx, ops, H):
    D = ops[SCORED[call]].shape[1] // H
    with np.errstate(all="ignore"):
        if call == "dot":
            return dot_attn_ref(ptr, idx, ops["q"], ops["k"], ops["v"], H, default_scale(D), block_edges=JUDGE_BLOCK)
        return gatv2_ref(ptr, idx, ops["xs"], ops["xd"], ops["a"], H, SLOPE, block_edges=JUDGE_BLOCK)


def head_scores(call, ptr, idx, ops, H):
    """float64 scores [E, H]"""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    with np.errstate(all="ignore"):
        if call == "dot":
            F = ops["q"].shape[1]
            t = ops["q"].astype(np.float64)[rows] * ops["k"].astype(np.float64)[idx]
            return float(default_scale(F // H)) * t.reshape(len(idx), H, -1).sum(axis=2)
        z = ops["xd"].astype(np.float64)[rows] + ops["xs"].astype(np.float64)[idx]
        zs = z * float(np.float32(SLOPE))
        return (ops["a"].astype(np.float64).reshape(1, -1) * np.where(z > zs, z, zs)).reshape(len(idx), H, -1).sum(axis=2)


def assert_spread(call, ptr, idx, ops, H, what):
    """the condition on the inputs: inside every (row, head) the finite scores lie within SPREAD of each other"""
    e = head_scores(call, ptr, idx, ops, H)
    hi, lo = np.where(np.isfinite(e), e, -np.inf), np.where(np.isfinite(e), e, np.inf)
    nz = np.flatnonzero(np.diff(ptr) > 0)
    starts = np.asarray(ptr)[nz].astype(np.intp)
    with np.errstate(invalid="ignore"):
        spread = np.maximum.reduceat(hi, starts, axis=0) - np.minimum.reduceat(lo, starts, axis=0)
    worst = float(np.nanmax(np.where(np.isfinite(spread), spread, 0.0))) if spread.size else 0.0
    assert worst < SPREAD, "%s: finite scores of one (row, head) spread by %.1f" % (what, worst)
    return worst


def masked_judge(call, ptr, idx, mask, masked_ops, H, h):
    """The judge of a masked case on head h's columns: (reference on the full graph [V, D] -- the class map --, reference, bound on the
    graph with the masked edges deleted, fully masked rows).  Asserts that the two references are one judge: equal bits wherever the row
    keeps an edge to 1e-7 of the bound (float64 rounding), apart from GATv2's column hD (0 * -Inf: the masked source row is the summed row),
    and NaN where it keeps none."""
    ptr_d, idx_d = delete_edges(ptr, idx, mask)
    ref_full, _, _ = head_ref(call, ptr, idx, masked_ops, H, h)
    ref_del, L, S = head_ref(call, ptr_d, idx_d, masked_ops, H, h)
    assert np.isfinite(ref_del).all() and np.isfinite(L).all()
    deg, deg_d = np.diff(ptr), np.diff(ptr_d)
    gone = (deg > 0) & (deg_d == 0)
    assert np.isnan(ref_full[gone]).all()
    bound = (dot_attn_bound if call == "dot" else gatv2_bound)(L, S, 1)
    # (numpy's reduceat does not add a row strictly in order, so the exact zeros of the masked edges can move the last bits of a float64
    # sum: equal to 1e-7 of the bound, that is 1e-12 (1 + L) S -- a few float64 roundings per edge of the longest row)
    with np.errstate(invalid="ignore"):
        same = np.abs(ref_full - ref_del) <= 1e-7 * bound
    if call == "v2":
        touched = deg_d < deg
        assert np.isnan(ref_full[touched, 0]).all()
        same[touched, 0] = True
    assert same[~gone].all(), "%s: the reference on the full graph is not the reference on the graph with the masked edges deleted" % call
    return ref_full, ref_del, bound, gone


def small_graph():
    """a cut of the GPU file's graph for the host checks: every short length, one single-segment and one 3-segment row"""
    lens = [0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 16, 33, LONG, LONG + 1, 2 * SEG + 1, 5]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    V = len(lens)
    n_src = V + 40
    rng = np.random.default_rng(4)
    return ptr, rng.integers(0, n_src, int(ptr[-1])).astype(np.int32), n_src


@pytest.mark.parametrize("call", ["dot", "v2"])
@pytest.mark.parametrize("pattern", PATTERNS, ids=pattern_id)
def test_masked_case_and_its_two_references(call, pattern):
    ptr, idx, n_src = small_graph()
    H, D, h = 3, 4, 1
    mask = mask_edges(ptr, pattern)
    idx2, clean, masked = masked_case(call, ptr, idx, n_src, H, D, h, mask, seed=20)
    V = len(ptr) - 1
    reserved = np.arange(n_src - N_RESERVED, n_src)
    assert np.array_equal(np.isin(idx2, reserved), mask) and idx2.min() >= 0 and idx2.max() < n_src
    e = head_scores(call, ptr, idx2, masked, H)
    assert np.isneginf(e[mask, h]).all() and np.isfinite(np.delete(e, h, axis=1)).all() and np.isfinite(e[~mask]).all()
    assert np.isfinite(head_scores(call, ptr, idx2, clean, H)).all()
    assert_spread(call, ptr, idx2, masked, H, pattern_id(pattern))
    ref_full, ref_del, bound, gone = masked_judge(call, ptr, idx2, mask, masked, H, h)
    # the head slice is the whole judge's head, and the other heads of the whole judge are the clean run's
    whole, whole_clean = full_ref(call, ptr, idx2, masked, H)[0], full_ref(call, ptr, idx2, clean, H)[0]
    assert np.array_equal(whole[:, h * D:(h + 1) * D], ref_full, equal_nan=True)
    other = np.r_[0:h * D, (h + 1) * D:H * D]
    assert np.array_equal(whole[:, other], whole_clean[:, other]) and np.isfinite(whole_clean).all()
    assert np.all(whole[np.diff(ptr) == 0] == 0)
    if pattern == "all":
        assert gone.sum() == (np.diff(ptr) > 0).sum()


def test_every_pattern_masks_what_it_says():
    ptr, _, _ = threshold_graph(n_src_extra=300)
    deg = np.diff(ptr)
    rows = np.repeat(np.arange(len(deg)), deg)
    count = lambda p: np.bincount(rows[mask_edges(ptr, p)], minlength=len(deg))
    for n in (1, 2, 3, 4, 5, 8):
        assert np.array_equal(count(("first", n)), np.minimum(deg, n))
    assert np.array_equal(count("all"), deg) and np.array_equal(count("all_but_last"), np.maximum(deg - 1, 0))
    assert np.array_equal(count("last"), np.minimum(deg, 1)) and np.array_equal(count("every_second"), (deg + 1) // 2)
    half = count("half_segment")
    assert (half[deg <= LONG] == 0).all() and (half[deg > LONG] > 0).all() and (half[deg > LONG] < np.minimum(deg, SEG)[deg > LONG]).all()
    for n in set(deg[deg > LONG].tolist()):
        n = min(n, SEG)
        for gpb in (4, 8):
            assert leading_half(n) % chunk_edges(n, gpb) == 0 or leading_half(n) > (gpb // 2) * chunk_edges(n, gpb)
            assert leading_half(n) >= chunk_edges(n, gpb)           # at least the whole first chunk
    assert leading_half(SEG) == SEG // 2
    multi = deg > SEG
    assert multi.sum() >= 3 and (deg == 3 * SEG + 37).any() and (deg == 2 * SEG + 1).any()
    first, mid, last = count(("segment", "first")), count(("segment", "middle")), count(("segment", "last"))
    assert (first[multi] == SEG).all() and (first[~multi] == 0).all()
    assert (mid[deg > 2 * SEG] == SEG).all() and (mid[deg <= 2 * SEG] == 0).all()
    assert np.array_equal(last[multi], (deg[multi] - 1) % SEG + 1) and (last[~multi] == 0).all()
    assert last[deg == 2 * SEG + 1][0] == 1 and last[deg == 3 * SEG + 37][0] == 37
    m = mask_edges(ptr, ("segment", "middle"))
    r = int(np.flatnonzero(deg == 3 * SEG + 37)[0])
    assert m[ptr[r] + 2 * SEG:ptr[r] + 3 * SEG].all() and m.sum() == SEG * (deg > 2 * SEG).sum()      # 4 segments: the third


@pytest.mark.parametrize("call", ["dot", "v2"])
@pytest.mark.parametrize("H,D", SHAPES)
def test_the_gpu_files_inputs_keep_their_scores_within_the_spread(call, H, D):
    ptr, idx, n_src = threshold_graph(n_src_extra=300)
    idx2, clean, _ = masked_case(call, ptr, idx, n_src, H, D, H // 2, np.zeros(len(idx), bool), seed=H * D)
    worst = assert_spread(call, ptr, idx2, clean, H, "%s %dx%d" % (call, H, D))
    print("%s %dx%d: widest spread of a (row, head) %.1f" % (call, H, D, worst))


# ------------------------------------------------------------------------------------------------ the online recurrence in fp32
f32 = np.float32


def _exp(x):
    with np.errstate(all="ignore"):
        return f32(np.exp(f32(x)))


def walk(e, x, batch, fixed):
    """gatv2_walk / dot_walk on one column: edges in batches, one guarded rescale per batch, then edge by edge.  (m, den, acc) in fp32.
    fixed = False is the walk before the fix: w = expf(e - m) with m = -Inf still."""
    m, den, acc = f32(NINF), f32(0), f32(0)
    with np.errstate(all="ignore"):
        for j in range(0, len(e), batch):
            eb, xb = e[j:j + batch], x[j:j + batch]
            bm = eb[0]
            for t in eb[1:]:
                bm = t if (np.isnan(bm) or t > bm) else bm      # fmaxf: a NaN operand loses
            if bm > m:
                sc = f32(0) if m == NINF else _exp(m - bm)
                den, acc, m = f32(den * sc), f32(acc * sc), bm
            ms = (f32(0) if m == NINF else m) if fixed else m
            for t, v in zip(eb, xb):
                w = _exp(f32(t - ms))
                den = f32(den + w)
                acc = f32(f32(v * w) + acc)
    return m, den, acc


def fold(triples, guard):
    """the fold of (m, den, acc) triples in ascending order: M = max m, den = sum den_g * expf(m_g - M).  guard: the LDS fold of a
    segment's chunks (m_g == -Inf: factor 0); without it: k_gatv2_merge over a row's segments"""
    with np.errstate(all="ignore"):
        M = f32(NINF)
        for m, _, _ in triples:
            M = m if (np.isnan(M) or m > M) else M
        d, o = f32(0), f32(0)
        for m, den, acc in triples:
            sc = f32(0) if (guard and m == NINF) else _exp(f32(m - M))
            d, o = f32(f32(den * sc) + d), f32(f32(acc * sc) + o)
    return M, d, o


def emulate_row(e, x, batch, gpb, fixed=True, guard=True):
    """y of one (row, head, column) as the kernels form it: a row up to 128 edges is one walk; a longer one is cut into segments of 512
    edges, each into gpb chunks of whole batches of 4, walked apart and folded; several segments are merged"""
    e, x = np.asarray(e, f32), np.asarray(x, f32)
    n = len(e)
    if n == 0:
        return f32(0)
    with np.errstate(all="ignore"):
        if n <= LONG:
            _, den, acc = walk(e, x, batch, fixed)
            return f32(acc / den)
        segs = []
        for b in range(0, n, SEG):
            es, xs = e[b:b + SEG], x[b:b + SEG]
            c = chunk_edges(len(es), gpb)
            segs.append(fold([walk(es[g * c:(g + 1) * c], xs[g * c:(g + 1) * c], batch, fixed) for g in range(gpb)], guard))
        _, den, acc = segs[0] if len(segs) == 1 else fold(segs, False)
        return f32(acc / den)


def row_judge(e, x):
    """the project's float64 judge on a one-row graph whose scores are e exactly (q = 1, k = e, one column, scale 1) and whose summed
    values are x; the bound from the row with its -Inf edges deleted"""
    e, x = np.asarray(e, f32), np.asarray(x, f32)
    n = len(e)
    run = lambda keep: dot_attn_ref(np.array([0, int(keep.sum())]), np.arange(int(keep.sum())), np.ones((1, 1), f32),
                                    e[keep].reshape(-1, 1), x[keep].reshape(-1, 1), 1, 1.0)
    with np.errstate(all="ignore"):
        y, _, _ = run(np.ones(n, bool))
        keep = ~np.isneginf(e)
        yd, L, S = run(keep) if keep.any() else (y, np.zeros((1, 1)), np.zeros((1, 1)))
    return float(y[0, 0]), float(yd[0, 0]), float(dot_attn_bound(L, S, 1)[0, 0])


def check_row(e, x, what, batches=(2, 4), gpbs=(4, 8)):
    y, yd, bound = row_judge(e, x)
    for batch in batches:
        for gpb in gpbs:
            got = emulate_row(e, x, batch, gpb)
            assert classes(got) == classes(y), "%s, batch %d, %d groups: %r against the judge's %r" % (what, batch, gpb, got, y)
            if np.isfinite(y):
                assert y == yd or np.isclose(y, yd, rtol=1e-15)
                assert abs(float(got) - yd) <= bound, "%s, batch %d, %d groups: |%r - %r| > %g" % (what, batch, gpb, got, yd, bound)
    return y


ROW_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 33, LONG, LONG + 1, SEG, SEG + 1, 2 * SEG + 37]


def one_row(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(f32) * f32(3), rng.standard_normal(n).astype(f32)


@pytest.mark.parametrize("pattern", PATTERNS, ids=pattern_id)
def test_the_fixed_recurrence_has_the_judges_class_on_every_pattern(pattern):
    for n in ROW_LENGTHS:
        e, x = one_row(n, n)
        mask = mask_edges(np.array([0, n]), pattern)
        e[mask] = NINF
        y = check_row(e, x, "%s, %d edges" % (pattern_id(pattern), n))
        assert np.isnan(y) == bool(mask.all())


def test_the_fixed_recurrence_has_the_judges_class_on_random_patterns_and_on_inf_and_nan():
    rng = np.random.default_rng(99)
    for trial in range(60):
        n = int(rng.choice(ROW_LENGTHS[:-3] + [LONG + 9]))
        e, x = one_row(n, 1000 + trial)
        e[rng.random(n) < rng.choice([0.2, 0.5, 0.9])] = NINF
        check_row(e, x, "random %d" % trial)
    for n in (1, 4, 5, 9, LONG + 1, SEG + 5):
        for pos in (0, n // 2, n - 1):
            for bad in (np.inf, np.nan):
                e, x = one_row(n, n)
                e[pos] = bad
                assert np.isnan(check_row(e, x, "%r at %d of %d" % (bad, pos, n)))
                e[:pos] = NINF      # ... behind masked edges too
                assert np.isnan(check_row(e, x, "%r at %d of %d behind masked edges" % (bad, pos, n)))
    # -Inf after a finite score was always right; so is a masked VALUE column in a masked edge: 0 * -Inf = NaN (GATv2's column hD)
    e, x = one_row(7, 5)
    e[3], x[3] = NINF, NINF
    assert np.isnan(check_row(e, x, "a masked edge whose summed value is -Inf"))


def test_the_recurrence_before_the_fix_gives_nan_where_a_batch_or_a_chunk_is_masked():
    """the regression's witness: the first FULL batch masked (4 edges at batch 4, 2 at batch 2), and a whole chunk of a segment masked"""
    e, x = np.array([NINF] * 4 + [1, 2, 0.5], f32), np.array([3, 1, 4, 1, 5, 9, 2], f32)
    y, _, _ = row_judge(e, x)
    w = np.exp(np.array([1, 2, 0.5]) - 2.0)
    assert abs(y - float((w * [5, 9, 2]).sum() / w.sum())) < 1e-12                  # the masked edges count for nothing
    old = lambda e, batch: emulate_row(e, x[:len(e)], batch, 4, fixed=False)
    assert np.isnan(old(e, 4)) and np.isnan(old(e, 2))
    e2 = np.array([NINF] * 2 + [1, 2, 0.5], f32)
    assert np.isfinite(old(e2, 4)) and np.isnan(old(e2, 2))
    e1 = np.array([NINF] + [1, 2, 0.5], f32)
    assert np.isfinite(old(e1, 4)) and np.isfinite(old(e1, 2))
    for batch in (2, 4):
        assert np.isfinite(emulate_row(e, x, batch, 4)) and np.isfinite(emulate_row(e2, x[:5], batch, 4))
        assert abs(float(emulate_row(e, x, batch, 4)) - y) < 1e-5 * 10
    # -Inf after a finite score, all -Inf, +Inf and NaN had the judge's class before the fix as well
    for ee in ([1, NINF, NINF, NINF, NINF, 2], [NINF] * 5, [1, np.inf, 2], [NINF, NINF, NINF, NINF, np.nan, 1]):
        ee = np.array(ee, f32)
        for batch in (2, 4):
            assert classes(old(ee, batch)) == classes(row_judge(ee, x[:len(ee)])[0])
    # a whole chunk masked: the second of the 4 (8) chunks of a 129-edge segment, every batch of it
    n = LONG + 1
    en, xn = one_row(n, 3)
    for gpb in (4, 8):
        c = chunk_edges(n, gpb)
        em = en.copy()
        em[c:2 * c] = NINF
        assert np.isfinite(row_judge(em, xn)[0])
        for batch in (2, 4):
            assert np.isnan(emulate_row(em, xn, batch, gpb, fixed=False))
            assert np.isfinite(emulate_row(em, xn, batch, gpb, fixed=True))
    # with the fix a masked chunk leaves (m, den, acc) = (-Inf, 0, 0), which the fold takes with or without its guard (expf(-Inf - M) = 0) ...
    em = en.copy()
    em[:chunk_edges(n, 4)] = NINF
    assert np.isfinite(emulate_row(em, xn, 4, 4, guard=True)) and np.isfinite(emulate_row(em, xn, 4, 4, guard=False))
    assert np.isnan(emulate_row(np.full(n, NINF, f32), xn, 4, 4))
    # ... but a whole masked SEGMENT of a row of several needs the guard: every chunk has m = -Inf, so M = -Inf and a plain
    # expf(-Inf - -Inf) leaves den = NaN in the segment's slot, which the merge's factor 0 does not clear.  With the guard the slot holds
    # (-Inf, 0, 0) and the merge's plain expf(-Inf - M) = 0 is enough: k_gatv2_merge needs no guard of its own.
    n = 2 * SEG + 37
    en, xn = one_row(n, 4)
    for lo, hi in ((0, SEG), (SEG, 2 * SEG), (2 * SEG, n)):
        em = en.copy()
        em[lo:hi] = NINF
        assert np.isnan(emulate_row(em, xn, 4, 4, fixed=False)) and np.isnan(emulate_row(em, xn, 4, 4, guard=False))
        assert np.isfinite(check_row(em, xn, "segment %d masked" % (lo // SEG)))


# ------------------------------------------------------------------------------------------------ what the GPU file expects of +Inf and NaN
@pytest.mark.parametrize("call", ["dot", "v2"])
@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
def test_the_judge_confines_an_inf_or_nan_score_to_the_row_heads_that_reach_it(call, bad):
    """group b of the GPU file states its expectation outright (NaN in exactly the (row, head)s that reach the element); here the judge says so"""
    ptr, idx, n_src = small_graph()
    H, D, h = 3, 4, 1
    V = len(ptr) - 1
    deg = np.diff(ptr)
    idx, reserved = reserve_sources(idx, n_src)
    special = int(reserved[0])
    rows = np.flatnonzero(deg > 0)[::3]
    idx[ptr[1:][rows] - 1] = special
    clean = attn_operands(call, V, n_src, H, D, h, seed=30)
    ref_clean = full_ref(call, ptr, idx, clean, H)[0]
    expect = np.zeros((V, H * D), bool)
    expect[rows, h * D:(h + 1) * D] = True
    ops = dict(clean)
    ops[SCORED[call]] = clean[SCORED[call]].copy()
    ops[SCORED[call]][special, h * D] = bad
    ref = full_ref(call, ptr, idx, ops, H)[0]
    assert np.array_equal(np.isnan(ref), expect) and np.array_equal(ref[~expect], ref_clean[~expect])
    # one element of the operand read once per row: that row's head only
    ops = dict(clean)
    ops[ROWWISE[call]] = clean[ROWWISE[call]].copy()
    ops[ROWWISE[call]][rows, h * D] = bad
    ref = full_ref(call, ptr, idx, ops, H)[0]
    assert np.array_equal(np.isnan(ref), expect) and np.array_equal(ref[~expect], ref_clean[~expect])
