"""GPU: Block.edgeconv / gnnagg_block_edgeconv_run (include/gnnagg.h section H, "Block EdgeConv layer") -- a two-layer MLP per edge and the
reduction per destination row in one launch.  The yardsticks: for fp32 and max the composition of existing calls
(Block.edgeconv(fused=False)), bit for bit; for fp32 sum / mean and for bf16 float64 over the stored operands.
The bound, per edge: with u = 2^-24, u16 = 2^-8 (bf16 operands; 0 for fp32), gamma_n = n u / (1 - n u), A_m = [|x_i|, |x_i| + |x_s|] (diff) or
|m| (cat), A_1 = A_m |W1| + |b1|, A_2 = A_1 |W2| + |b2|:  |msg - ref| <= ((1 + gamma_n)(1 + u16)^2 - 1 + 1e-5) A_2 + 1e-30 with n = Kp + Hp + 8
(2 F and H rounded up to 32) + the longest row for sum and mean -- every term of out passes at most n fp32 roundings and the two bf16
roundings of the difference and of z, ReLU is 1-Lipschitz, 1e-5 is the project's slack for the MFMA's internal order.  A row's bound is the
sum of its edges' bounds (mean: / degree; max: the largest of them); a bf16 out adds u16 (|ref| + bound) for its one rounding.
Measured on one MI355X (profiles/block_edgeconv/gpu_tests_output.txt): the worst |out - ref| / bound of this file is 0.187 for bf16
operands (a bf16 out, diff, sum), 0.126 for bf16 past the grid cap and 0.004 for fp32 sum / mean."""
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc

import block_run_ref as br
from test_gpu_block_sage import B16, DEV, F32, SB, dev, same_bits, tblock

pytestmark = pytest.mark.gpu
COMBINES = ["diff", "cat"]


@functools.lru_cache(maxsize=None)
def operands(F, H, N, dt, ints=False):
    """x [NUM_X, F], W1 [2 F, H], W2 [H, N] of dt, b1, b2: on the device, shared and never written"""
    rng = np.random.default_rng(10000 * F + 100 * H + N)
    draw = (lambda lo, hi, s: rng.integers(lo, hi + 1, s)) if ints else (lambda lo, hi, s: rng.standard_normal(s))
    x, w1, w2, b1, b2 = draw(-4, 4, (br.NUM_X, F)), draw(-1, 1, (2 * F, H)), draw(-1, 1, (H, N)), draw(-3, 3, H), draw(-3, 3, N)
    f = lambda a: dev(a.astype(np.float32))
    return f(x).to(dt), f(w1).to(dt), f(w2).to(dt), f(b1), f(b2)


def judge(blk, x, w1, w2, b1=None, b2=None, combine="diff", reduce="max", relu=False):
    """float64 over the stored operands: (out, bound, the largest |m| and |z|)"""
    n, F, H, N = blk.num_dst, x.shape[1], w1.shape[1], w2.shape[1]
    deg = (blk.ptr[1:] - blk.ptr[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), deg)
    src, xd = blk.src_nodes.long(), x.double()
    xi, xs = xd[src[rows]], xd[src[blk.idx.long()]]
    m = torch.cat([xi, xs - xi if combine == "diff" else xs], 1)
    a_m = torch.cat([xi.abs(), xi.abs() + xs.abs() if combine == "diff" else xs.abs()], 1)
    z, a_1 = m @ w1.double(), a_m @ w1.double().abs()
    if b1 is not None:
        z, a_1 = z + b1.double(), a_1 + b1.double().abs()
    z = z.clamp_min(0)
    msg, a_2 = z @ w2.double(), a_1 @ w2.double().abs()
    if b2 is not None:
        msg, a_2 = msg + b2.double(), a_2 + b2.double().abs()
    nu = (-(-2 * F // 32) * 32 + -(-H // 32) * 32 + 8 + (0 if reduce == "max" else int(deg.max()))) * 2.0 ** -24
    u16 = 2.0 ** -8 if x.dtype == B16 else 0.0
    eb = ((1 + nu / (1 - nu)) * (1 + u16) ** 2 - 1 + 1e-5) * a_2 + 1e-30
    zero, at = torch.zeros((n, N), device=DEV, dtype=torch.float64), rows[:, None].expand(-1, N)
    if reduce == "max":
        o = torch.full_like(zero, -np.inf).scatter_reduce_(0, at, msg, "amax")
        o[deg == 0] = 0
        bound = zero.clone().scatter_reduce_(0, at, eb, "amax") + 1e-30
    else:
        o, bound = zero.clone().index_add_(0, rows, msg), zero.clone().index_add_(0, rows, eb) + 1e-30
        if reduce == "mean":
            o, bound = o / deg.clamp_min(1)[:, None], bound / deg.clamp_min(1)[:, None]
    largest = float(torch.cat([m.abs().reshape(-1), z.reshape(-1), m.new_zeros(1)]).max())   # (a block may have no edge)
    return (o.clamp_min(0) if relu else o), bound, largest


def check_bound(out, ref, bound, what):
    if out.dtype == B16:
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)
    err = (out.double() - ref).abs()
    print("%s: worst |out - ref| / bound = %.4f" % (what, float((err / bound).max())))
    assert (err <= bound).all().item(), what


@pytest.mark.parametrize("combine", COMBINES)
@pytest.mark.parametrize("F,H,N", [(1, 1, 1), (3, 5, 15), (4, 16, 16), (20, 17, 33), (33, 47, 20), (64, 64, 128), (128, 128, 47)])
def test_fp32_max_is_the_composition_of_the_existing_calls_bit_for_bit(F, H, N, combine):
    blk = tblock()
    x, w1, w2, b1, b2 = operands(F, H, N, F32)
    x_src = x[blk.src_nodes.long()].contiguous()
    everything = dict(b1=b1, b2=b2, relu=True)
    variants = [everything] + [{k: v for k, v in everything.items() if k != drop} for drop in everything] + [dict(everything, gathered=True)]
    for v in variants:
        xx, kw = (x_src if v.get("gathered") else x), dict(v, combine=combine, reduce="max")
        assert same_bits(blk.edgeconv(xx, w1, w2, fused=True, **kw), blk.edgeconv(xx, w1, w2, fused=False, **kw)), sorted(v)
    assert same_bits(gnc.block_edgeconv_run(blk, x, w1, w2, b1, b2, combine=combine, fused=True), blk.edgeconv(x, w1, w2, b1, b2, combine=combine, fused=False))


@pytest.mark.parametrize("combine", COMBINES)
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("F,H,N", [(3, 5, 15), (20, 17, 33), (64, 64, 128)])
def test_fp32_sum_and_mean_are_inside_the_derived_float64_bound(F, H, N, reduce, combine):
    blk = tblock()
    x, w1, w2, b1, b2 = operands(F, H, N, F32)
    kw = dict(b1=b1, b2=b2, combine=combine, reduce=reduce)
    plain = blk.edgeconv(x, w1, w2, fused=True, **kw)
    check_bound(plain, *judge(blk, x, w1, w2, **kw)[:2], what="fp32 %s %s" % (reduce, combine))
    assert torch.equal(blk.edgeconv(x, w1, w2, relu=True, fused=True, **kw), plain.clamp_min(0))


@pytest.mark.parametrize("combine", COMBINES)
@pytest.mark.parametrize("odt", [F32, B16], ids=["out_fp32", "out_bf16"])
@pytest.mark.parametrize("F,H,N", [(1, 1, 1), (3, 64, 64), (8, 8, 8), (31, 33, 17), (64, 64, 64), (128, 128, 47)])
def test_bf16_is_inside_the_derived_float64_bound(F, H, N, odt, combine):
    blk = tblock()
    x, w1, w2, b1, b2 = operands(F, H, N, B16)
    for kw in (dict(b1=b1, b2=b2, reduce="max"), dict(reduce="sum"), dict(b1=b1, reduce="mean")):
        kw = dict(kw, combine=combine)
        plain = blk.edgeconv(x, w1, w2, out_dtype=odt, fused=True, **kw)
        check_bound(plain, *judge(blk, x, w1, w2, **kw)[:2], what="%s %s" % (odt, sorted(kw.items())[-2:]))
        assert torch.equal(blk.edgeconv(x, w1, w2, out_dtype=odt, relu=True, fused=True, **kw), plain.clamp_min(0))


@pytest.mark.parametrize("reduce,combine", [("max", "diff"), ("sum", "cat")])
def test_small_integers_are_exact_in_bf16(reduce, combine):
    blk = tblock()
    x, w1, w2, b1, b2 = operands(8, 12, 17, B16, ints=True)
    ref, _, largest = judge(blk, x, w1, w2, b1, b2, combine=combine, reduce=reduce)
    assert largest <= 256                                        # m and z are integers bf16 holds: both roundings are exact
    assert torch.equal(blk.edgeconv(x, w1, w2, b1, b2, combine=combine, reduce=reduce, out_dtype=F32, fused=True).double(), ref)


@pytest.mark.parametrize("dt,F,H,N", [(F32, 3, 5, 15), (B16, 8, 8, 8)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, "past the grid cap"])
def test_row_block_and_tile_edges(n, dt, F, H, N):
    if n == "past the grid cap":   # every workgroup of the capped grid takes a second row block, some a third
        cap = gnc.lib().gnnagg_block_edgeconv_grid_cap(0, F, H, N, gnc.aggregator.FEATURE_DTYPES[dt])
        assert cap > 0
        n = 16 * (2 * cap + 3) + 5
    blk = tblock(n)
    x, w1, w2, b1, b2 = operands(F, H, N, dt)
    kw = dict(b1=b1, b2=b2, relu=True, reduce="max" if dt == F32 else "mean")
    out = blk.edgeconv(x, w1, w2, fused=True, **kw)
    assert tuple(out.shape) == (n, N)
    if dt == F32:
        assert same_bits(out, blk.edgeconv(x, w1, w2, fused=False, **kw))
    else:
        check_bound(out, *judge(blk, x, w1, w2, **kw)[:2], what="num_dst = %d" % n)


@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
def test_pitch_canaries_nan_containment_and_graph_capture(dt):
    blk = tblock()
    F, H, N = 36, 20, 24
    x, w1, w2, b1, b2 = operands(F, H, N, dt)
    kw = dict(b1=b1, b2=b2, relu=True, fused=True)
    base = blk.edgeconv(x, w1, w2, **kw)
    assert torch.isfinite(base).all().item()
    for pad, off in ((16, 4), (13, 1)):                          # pitched column views of x: narrower lanes, several column tiles per row
        xv = torch.zeros((br.NUM_X, F + pad), device=DEV, dtype=dt)[:, off:off + F]
        xv.copy_(x)
        assert not xv.is_contiguous() and same_bits(blk.edgeconv(xv, w1, w2, **kw), base), (pad, off)
    n, guard = blk.num_dst * N, 256                              # out inside a NaN-filled buffer
    buf = torch.full((n + 2 * guard,), float("nan"), device=DEV, dtype=dt)
    out = blk.edgeconv(x, w1, w2, out=buf[guard:guard + n].view(blk.num_dst, N), **kw)
    assert same_bits(out, base) and buf[:guard].isnan().all().item() and buf[guard + n:].isnan().all().item()
    # a NaN source row reaches the rows that see it, as a neighbour or as their own row, and nobody else in their edge tiles
    a = int(SB["idx"][SB["idx"] < blk.num_dst][0])               # somebody's neighbour, and the self row of destination a
    dirty = x.clone()
    dirty[int(SB["src_nodes"][a])] = float("nan")
    hit = dev(np.array([(i == a and SB["ptr"][i] < SB["ptr"][i + 1]) or bool((SB["idx"][SB["ptr"][i]:SB["ptr"][i + 1]] == a).any())
                        for i in range(blk.num_dst)]))
    assert 1 < int(hit.sum()) < blk.num_dst
    for reduce in ("sum", "mean", "max"):
        clean, got = blk.edgeconv(x, w1, w2, reduce=reduce, **kw), blk.edgeconv(dirty, w1, w2, reduce=reduce, **kw)
        assert got[hit].isnan().all().item() and same_bits(got[~hit], clean[~hit]), reduce
    # a captured launch replays to the eager bits
    x2 = operands(F, H, N + 1, dt)[0]
    want2 = blk.edgeconv(x2, w1, w2, **kw)
    xs, out = x.clone(), torch.full((blk.num_dst, N), 7.0, device=DEV, dtype=dt)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        blk.edgeconv(xs, w1, w2, out=out, **kw)
    assert out.eq(7.0).all().item()                              # captured, not run
    for xin, want in ((x2, want2), (x, base), (x2, want2)):
        xs.copy_(xin)                                            # in place: the graph reads the same addresses
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want)
