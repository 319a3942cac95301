"""GPU: Block.gin / gnnagg_block_gin_run (include/gnnagg.h section F, "Block GIN layer") -- aggregate + two-layer MLP in one launch.
The yardsticks: for fp32 the composition of existing calls (Block.gin(fused=False)), bit for bit; for bf16 float64 over the stored operands.
The bf16 bound: with u = 2^-24, u16 = 2^-8, gamma_n = n u / (1 - n u), A_h = |1 + eps| |x_dst| + sum_p |s_p| |x_src(p)| (mean: s_p carries
1 / deg), A_1 = A_h |W1| + |b1|, A_2 = A_1 |W2| + |b2|:  |out - ref| <= ((1 + gamma_n)(1 + u16)^2 - 1 + 1e-5) A_2 + 1e-30 with n = the longest
row + Fp + Hp + 8 -- every term of out passes at most n fp32 roundings and the two bf16 roundings of h and z, ReLU is 1-Lipschitz, 1e-5 is
the project's slack for the MFMA's internal order -- and a bf16 out adds u16 (|ref| + bound) for its one rounding.  Measured on one MI355X:
the worst |out - ref| / bound of this file is 0.238 (bf16 out) and 0.181 (fp32 out), both at 1 -> 1 -> 1."""
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc

import block_run_ref as br
from test_gpu_block_sage import B16, DEV, F32, SB, dev, same_bits, tblock

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def operands(F, H, N, dt, ints=False):
    """x [NUM_X, F], W1 [F, H], W2 [H, N] of dt, b1, b2, val per block edge and per full edge: on the device, shared and never written"""
    rng = np.random.default_rng(10000 * F + 100 * H + N)
    draw = (lambda lo, hi, s: rng.integers(lo, hi + 1, s)) if ints else (lambda lo, hi, s: rng.standard_normal(s))
    x, w1, w2, b1, b2 = draw(-4, 4, (br.NUM_X, F)), draw(-1, 1, (F, H)), draw(-1, 1, (H, N)), draw(-3, 3, H), draw(-3, 3, N)
    full = rng.standard_normal(br.NUM_E_FULL).astype(np.float32)
    f = lambda a: dev(a.astype(np.float32))
    return f(x).to(dt), f(w1).to(dt), f(w2).to(dt), f(b1), f(b2), dev(full[SB["eid"]]), dev(full)


def judge(blk, x, w1, w2, b1=None, b2=None, eps=0.0, reduce="sum", val=None, relu=False):
    """float64 over the stored operands: (out, bound, the largest |h| and |z|)"""
    n, F, H = blk.num_dst, x.shape[1], w1.shape[1]
    deg = (blk.ptr[1:] - blk.ptr[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), deg)
    s = torch.ones(blk.num_edges, device=DEV, dtype=torch.float64) if val is None else val.double()
    if reduce == "mean":
        s = s / deg[rows]
    t = x.double()[blk.src_nodes.long()[blk.idx.long()]] * s[:, None]
    zero = torch.zeros((n, F), device=DEV, dtype=torch.float64)
    if reduce == "max":   # over the exact products: no chain error
        agg = torch.full_like(zero, -np.inf).scatter_reduce_(0, rows[:, None].expand(-1, F), t, "amax")
        agg[deg == 0] = 0
    else:
        agg = zero.clone().index_add_(0, rows, t)
    sc, x_dst = float(np.float32(1.0 + eps)), x.double()[blk.src_nodes.long()[:n]]
    h, a_h = sc * x_dst + agg, abs(sc) * x_dst.abs() + zero.clone().index_add_(0, rows, t.abs())
    z, a_1 = h @ w1.double(), a_h @ w1.double().abs()
    if b1 is not None:
        z, a_1 = z + b1.double(), a_1 + b1.double().abs()
    z = z.clamp_min(0)
    o, a_2 = z @ w2.double(), a_1 @ w2.double().abs()
    if b2 is not None:
        o, a_2 = o + b2.double(), a_2 + b2.double().abs()
    nu = (int(deg.max()) + -(-F // 32) * 32 + -(-H // 32) * 32 + 8) * 2.0 ** -24
    bound = ((1 + nu / (1 - nu)) * (1 + 2.0 ** -8) ** 2 - 1 + 1e-5) * a_2 + 1e-30
    return (o.clamp_min(0) if relu else o), bound, max(float(h.abs().max()), float(z.abs().max()))


def check_bound(out, ref, bound, what):
    if out.dtype == B16:
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)
    err = (out.double() - ref).abs()
    print("%s: worst |out - ref| / bound = %.4f" % (what, float((err / bound).max())))
    assert (err <= bound).all().item(), what


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("F,H,N", [(1, 1, 1), (3, 5, 15), (4, 16, 16), (20, 17, 33), (33, 47, 20), (100, 128, 47), (256, 256, 16)])
def test_fp32_is_the_composition_of_the_existing_calls_bit_for_bit(F, H, N, reduce):
    blk = tblock()
    x, w1, w2, b1, b2, val, full = operands(F, H, N, F32)
    x_src = x[blk.src_nodes.long()].contiguous()
    everything = dict(b1=b1, b2=b2, val=val, relu=True, eps=0.25)
    variants = [everything] + [{k: v for k, v in everything.items() if k != drop} for drop in everything]   # (eps dropped: eps = 0)
    variants += [dict(everything, val=full, val_full=True), dict(everything, gathered=True)]
    for v in variants:
        xx = x_src if v.get("gathered") else x
        assert same_bits(blk.gin(xx, w1, w2, reduce=reduce, fused=True, **v), blk.gin(xx, w1, w2, reduce=reduce, fused=False, **v)), sorted(v)
    assert same_bits(gnc.block_gin_run(blk, x, w1, w2, b1, b2, reduce=reduce), blk.gin(x, w1, w2, b1, b2, reduce=reduce, fused=False))


@pytest.mark.parametrize("odt", [F32, B16], ids=["out_fp32", "out_bf16"])
@pytest.mark.parametrize("F,H,N", [(1, 1, 1), (8, 8, 8), (31, 33, 17), (32, 64, 64), (100, 17, 128), (128, 128, 128)])
def test_bf16_is_inside_the_derived_float64_bound(F, H, N, odt):
    blk = tblock()
    x, w1, w2, b1, b2, val, _ = operands(F, H, N, B16)
    for kw in (dict(b1=b1, b2=b2, val=val, eps=0.25, reduce="mean"), dict(reduce="sum"), dict(b1=b1, eps=-0.5, reduce="max")):
        plain = blk.gin(x, w1, w2, out_dtype=odt, fused=True, **kw)
        check_bound(plain, *judge(blk, x, w1, w2, **kw)[:2], what="%s %s" % (odt, sorted(kw)))
        assert torch.equal(blk.gin(x, w1, w2, out_dtype=odt, relu=True, fused=True, **kw), plain.clamp_min(0))


def test_small_integers_are_exact_in_bf16():
    blk = tblock()
    x, w1, w2, b1, b2, _, _ = operands(20, 40, 17, B16, ints=True)
    ref, _, largest = judge(blk, x, w1, w2, b1, b2, eps=1.0, reduce="max")
    assert largest <= 256                                        # h and z are integers bf16 holds: both roundings are exact
    assert torch.equal(blk.gin(x, w1, w2, b1, b2, eps=1.0, reduce="max", out_dtype=F32, fused=True).double(), ref)


@pytest.mark.parametrize("dt,F,H,N", [(F32, 20, 17, 33), (B16, 40, 24, 24)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, "past the grid cap"])
def test_row_tile_edges_and_both_copies_of_tile_rows(n, dt, F, H, N):
    if n == "past the grid cap":   # every workgroup of the capped grid takes a second tile, some a third
        cap = gnc.lib().gnnagg_block_gin_grid_cap(F, H, N, gnc.aggregator.FEATURE_DTYPES[dt])
        assert cap > 0
        n = 16 * (2 * cap + 3) + 5
    blk = tblock(n)
    x, w1, w2, b1, b2, _, _ = operands(F, H, N, dt)
    kw = dict(b1=b1, b2=b2, eps=0.25, reduce="mean", relu=True)
    out = blk.gin(x, w1, w2, fused=True, **kw)
    assert tuple(out.shape) == (n, N)
    if dt == F32:
        assert same_bits(out, blk.gin(x, w1, w2, fused=False, **kw))
    else:
        check_bound(out, *judge(blk, x, w1, w2, **kw)[:2], what="num_dst = %d" % n)


@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
def test_pitch_canaries_nan_containment_and_graph_capture(dt):
    blk = tblock()
    F, H, N = 36, 20, 24
    x, w1, w2, b1, b2, val, _ = operands(F, H, N, dt)
    kw = dict(b1=b1, b2=b2, eps=0.25, reduce="mean", val=val, relu=True, fused=True)
    base = blk.gin(x, w1, w2, **kw)
    assert torch.isfinite(base).all().item()
    for pad, off in ((16, 4), (13, 1)):                          # pitched column views of x: narrower lanes, several column tiles per row
        xv = torch.zeros((br.NUM_X, F + pad), device=DEV, dtype=dt)[:, off:off + F]
        xv.copy_(x)
        assert not xv.is_contiguous() and same_bits(blk.gin(xv, w1, w2, **kw), base), (pad, off)
    n, guard = blk.num_dst * N, 256                              # out inside a NaN-filled buffer
    buf = torch.full((n + 2 * guard,), float("nan"), device=DEV, dtype=dt)
    out = blk.gin(x, w1, w2, out=buf[guard:guard + n].view(blk.num_dst, N), **kw)
    assert same_bits(out, base) and buf[:guard].isnan().all().item() and buf[guard + n:].isnan().all().item()
    # a NaN source row reaches the rows that see it, through both products, and nobody else in their MFMA tile
    a = int(SB["idx"][SB["idx"] < blk.num_dst][0])               # somebody's neighbour, and the self row of destination a
    dirty = x.clone()
    dirty[int(SB["src_nodes"][a])] = float("nan")
    hit = dev(np.array([i == a or bool((SB["idx"][SB["ptr"][i]:SB["ptr"][i + 1]] == a).any()) for i in range(blk.num_dst)]))
    got = blk.gin(dirty, w1, w2, **kw)
    assert 1 < int(hit.sum()) < blk.num_dst and got[hit].isnan().all().item() and same_bits(got[~hit], base[~hit])
    # a captured launch replays to the eager bits
    x2 = operands(F, H, N + 1, dt)[0]
    want2 = blk.gin(x2, w1, w2, **kw)
    xs, out = x.clone(), torch.full((blk.num_dst, N), 7.0, device=DEV, dtype=dt)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        blk.gin(xs, w1, w2, out=out, **kw)
    assert out.eq(7.0).all().item()                              # captured, not run
    for xin, want in ((x2, want2), (x, base), (x2, want2)):
        xs.copy_(xin)                                            # in place: the graph reads the same addresses
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want)
