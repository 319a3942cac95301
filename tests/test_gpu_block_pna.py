"""GPU: Block.pna / gnnagg_block_pna_run (include/gnnagg.h section F, "Block PNA layer") -- multi-aggregation + combine in one launch.
The yardsticks: for fp32 the composition of existing calls (Block.pna(fused=False): gather, run_multi, cat, matmul_NN), bit for bit on rows
of at most 128 edges; for bf16, and for the longer rows, float64 over the stored operands.
The bound, from the run_multi contract: aggregate a carries e_a = 1e-5 sum|m| (sum), that / d (mean), 4e-5 S2 / d (var), sqrt of var's (std:
|sqrt p - sqrt q| <= sqrt|p - q|), 0 (min, max); its tile value one bf16 rounding more, e_a + u16 (|a| + e_a) with u16 = 2^-8; the row's fp32
scalar (logf, one division, delta's conversion: 2^-21 relative) multiplies it in fp32.  With T = |x_dst| |W_self| + sum scaler |a| |W| + |bias|
and E = sum scaler (e_a + u16 (|a| + e_a)) |W|:  |out - ref| <= E + (gamma_n + 1e-5 + 2^-21) (T + E) + 1e-30, gamma_n = n u / (1 - n u),
u = 2^-24, n = (1 + S A) Fp + 8 fp32 roundings per element (Fp = feat rounded up to 32), 1e-5 the project's slack for the MFMA's internal
order; ReLU is 1-Lipschitz; a bf16 out adds u16 (|ref| + bound) for its one rounding.  Measured on one MI355X: the worst |out - ref| / bound
of this file is 0.959 with a bf16 out (u16 is attained: half an ulp of a value just above a power of two), 0.834 with a fp32 out of bf16
operands (at 1 -> 1, where one rounding is the whole error; below 0.4 from 31 -> 17 on) and 0.0065 for fp32 operands (rows of 129 and 300
edges included)."""
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd.aggregator import AGGRS, SCALERS

import block_run_ref as br
from test_gpu_block_gin import check_bound
from test_gpu_block_sage import B16, DEV, F32, SB, dev, same_bits, tblock

pytestmark = pytest.mark.gpu
DELTA = gnc.pna_delta(SB["ptr"])
DEFAULT, ALL_A, ALL_S = ("mean", "min", "max", "std"), tuple(AGGRS), tuple(SCALERS)
MASKS = [(DEFAULT, ("identity",)), (ALL_A, ALL_S), (("sum",), ("attenuation",)), (("var",), ("identity", "amplification"))]


@functools.lru_cache(maxsize=None)
def operands(F, N, slabs, dt, ints=False):
    """x [NUM_X, F], W [slabs * F, N], W_self [F, N] of dt, bias [N], val per block edge and per full edge: on the device, shared, never written"""
    rng = np.random.default_rng(10000 * F + 100 * N + slabs)
    draw = (lambda lo, hi, s: rng.integers(lo, hi + 1, s)) if ints else (lambda lo, hi, s: rng.standard_normal(s))
    x, w, ws, b = draw(-4, 4, (br.NUM_X, F)), draw(-1, 1, (slabs * F, N)), draw(-1, 1, (F, N)), draw(-3, 3, N)
    full = rng.standard_normal(br.NUM_E_FULL).astype(np.float32)
    f = lambda a: dev(a.astype(np.float32))
    return f(x).to(dt), f(w).to(dt), f(ws).to(dt), f(b), dev(full[SB["eid"]]), dev(full)


def judge(blk, x, w, w_self=None, bias=None, aggrs=DEFAULT, scalers=("identity",), delta=None, val=None, relu=False, **_):
    """float64 over the stored operands: (out, bound, the largest |tile value|)"""
    n, F = blk.num_dst, x.shape[1]
    deg = (blk.ptr[1:] - blk.ptr[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), deg)
    m = x.double()[blk.src_nodes.long()[blk.idx.long()]]
    if val is not None:
        m = m * val.double()[:, None]
    zero = torch.zeros((n, F), device=DEV, dtype=torch.float64)
    add = lambda t: zero.clone().index_add_(0, rows, t)
    ext = lambda how, seed: torch.full_like(zero, seed).scatter_reduce_(0, rows[:, None].expand(-1, F), m, how)
    d, live = deg.clamp_min(1).double()[:, None], (deg > 0)[:, None]
    s1, sa, s2 = add(m), add(m.abs()), add(m * m)
    var = (s2 / d - (s1 / d) ** 2).clamp_min(0)
    table = {"sum": (s1, 1e-5 * sa), "mean": (s1 / d, 1e-5 * sa / d), "min": (ext("amin", np.inf), zero), "max": (ext("amax", -np.inf), zero),
             "var": (var, 4e-5 * s2 / d), "std": (var.sqrt(), (4e-5 * s2 / d).sqrt())}
    lg = torch.log(deg.double() + 1)[:, None]
    scale = {"identity": torch.ones_like(lg), "amplification": lg / (delta or 1.0), "attenuation": (delta or 1.0) / lg}
    val_, abs_, err_ = [], [], []
    for s in sorted(scalers, key=SCALERS.get):          # scaler-major, ascending bit order
        for a in sorted(aggrs, key=AGGRS.get):
            v, e = table[a]
            val_.append(torch.where(live, v * scale[s], zero))
            abs_.append(val_[-1].abs())
            err_.append(torch.where(live, (e + 2.0 ** -8 * (v.abs() + e)) * scale[s], zero))
    x_dst = x.double()[blk.src_nodes.long()[:n]]
    ref, t, e = torch.cat(val_, 1) @ w.double(), torch.cat(abs_, 1) @ w.double().abs(), torch.cat(err_, 1) @ w.double().abs()
    if w_self is not None:
        ref, t = ref + x_dst @ w_self.double(), t + x_dst.abs() @ w_self.double().abs()
    if bias is not None:
        ref, t = ref + bias.double(), t + bias.double().abs()
    nu = ((1 + len(val_)) * -(-F // 32) * 32 + 8) * 2.0 ** -24
    bound = e + (nu / (1 - nu) + 1e-5 + 2.0 ** -21) * (t + e) + 1e-30
    tiles = torch.stack([torch.where(live, table[a][0], zero).abs().max() for a in aggrs])
    return (ref.clamp_min(0) if relu else ref), bound, float(tiles.max())


def short_rows(blk):
    return (blk.ptr[1:] - blk.ptr[:-1]) <= 128           # the rows run_multi walks with one lane group, as this kernel walks every row


@pytest.mark.parametrize("aggrs,scalers", MASKS, ids=["default", "all", "sum_att", "var_id_amp"])
@pytest.mark.parametrize("F,N", [(1, 1), (3, 15), (4, 16), (20, 33), (33, 20), (100, 47), (256, 16)])
def test_fp32_is_the_composition_of_the_existing_calls(F, N, aggrs, scalers):
    blk = tblock()
    x, w, ws, b, val, full = operands(F, N, len(aggrs) * len(scalers), F32)
    x_src, short = x[blk.src_nodes.long()].contiguous(), short_rows(blk)
    assert 0 < int(short.sum()) < blk.num_dst
    everything = dict(w_self=ws, bias=b, val=val, relu=True)
    variants = [everything] + [{k: v for k, v in everything.items() if k != drop} for drop in everything]
    variants += [dict(everything, val=full, val_full=True), dict(everything, gathered=True)]
    for v in variants:
        kw = dict(v, aggrs=aggrs, scalers=scalers, delta=DELTA)
        xx = x_src if v.get("gathered") else x
        got, want = blk.pna(xx, w, fused=True, **kw), blk.pna(xx, w, fused=False, **kw)
        assert same_bits(got[short], want[short]), sorted(v)
        val_blk = full[blk.eid.long()] if v.get("val_full") else v.get("val")
        check_bound(got, *judge(blk, x, w, **dict(kw, val=val_blk))[:2], what="fp32, long rows too, %s" % sorted(v))
    w4 = operands(F, N, 4, F32)[1]                                # the function form, with the default masks
    assert same_bits(gnc.block_pna_run(blk, x, w4, ws, b)[short], blk.pna(x, w4, ws, b, fused=False)[short])


@pytest.mark.parametrize("odt", [F32, B16], ids=["out_fp32", "out_bf16"])
@pytest.mark.parametrize("F,N", [(1, 1), (8, 8), (31, 17), (32, 64), (100, 128), (128, 64)])
def test_bf16_is_inside_the_derived_float64_bound(F, N, odt):
    blk = tblock()
    masks = [m for m in MASKS if gnc.block_pna_supported(F, N, len(m[0]), len(m[1]), B16)]   # (the image of the widest ones is past the LDS)
    assert len(masks) >= (2 if F >= 100 else 4)
    for aggrs, scalers in masks:
        x, w, ws, b, val, _ = operands(F, N, len(aggrs) * len(scalers), B16)
        for kw in (dict(w_self=ws, bias=b, val=val), dict()):
            kw = dict(kw, aggrs=aggrs, scalers=scalers, delta=DELTA)
            plain = blk.pna(x, w, out_dtype=odt, fused=True, **kw)
            check_bound(plain, *judge(blk, x, w, **kw)[:2], what="%s %s x %s" % (odt, aggrs, scalers))
            assert torch.equal(blk.pna(x, w, out_dtype=odt, relu=True, fused=True, **kw), plain.clamp_min(0))


@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
def test_a_row_without_edges_keeps_its_zeros_under_attenuation(dt):
    blk = tblock()
    assert int(blk.ptr[1]) == 0                                   # row 0 has no edges: delta / logf(1) would be +Inf, 0 * Inf a NaN
    x, w, ws, b, _, _ = operands(36, 24, 8, dt)
    for relu in (False, True):
        out = blk.pna(x, w, ws, b, scalers=("identity", "attenuation"), delta=DELTA, relu=relu, fused=True)
        alone = blk.sage(x, w[:36].contiguous(), ws, b, relu=relu, fused=True)   # another kernel: row 0 is act(x_dst . W_self + 0 + bias)
        assert torch.isfinite(out).all().item() and same_bits(out[:1], alone[:1])


@pytest.mark.parametrize("F,N", [(20, 33), (128, 64)])
def test_fp32_mean_alone_has_the_bits_of_block_sage(F, N):
    blk = tblock()
    x, w, ws, b, _, _ = operands(F, N, 1, F32)
    assert same_bits(blk.pna(x, w, ws, b, aggrs=("mean",), fused=True), blk.sage(x, w, ws, b, reduce="mean", fused=True))


def test_small_integers_are_exact_in_bf16():
    blk = tblock()
    x, w, ws, b, _, _ = operands(20, 17, 3, B16, ints=True)
    ref, _, largest = judge(blk, x, w, ws, b, aggrs=("sum", "min", "max"))
    assert largest <= 256                                        # integers bf16 holds: the tile's rounding is exact
    assert torch.equal(blk.pna(x, w, ws, b, aggrs=("sum", "min", "max"), out_dtype=F32, fused=True).double(), ref)


@pytest.mark.parametrize("dt,F,N", [(F32, 20, 33), (B16, 40, 24)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, "past the grid cap"])
def test_row_tile_edges_and_the_per_tile_scalars(n, dt, F, N):
    scalers = ("identity", "amplification")                      # a row scalar left over from another tile would show
    if n == "past the grid cap":   # every workgroup of the capped grid takes a second tile, some a third
        cap = gnc.lib().gnnagg_block_pna_grid_cap(F, N, 4, 2, gnc.aggregator.FEATURE_DTYPES[dt])
        assert cap > 0
        n = 16 * (2 * cap + 3) + 5
    blk = tblock(n)
    x, w, ws, b, _, _ = operands(F, N, 8, dt)
    kw = dict(w_self=ws, bias=b, scalers=scalers, delta=DELTA, relu=True)
    out = blk.pna(x, w, fused=True, **kw)
    assert tuple(out.shape) == (n, N)
    if dt == F32:
        short = short_rows(blk)
        assert same_bits(out[short], blk.pna(x, w, fused=False, **kw)[short])
    check_bound(out, *judge(blk, x, w, **kw)[:2], what="num_dst = %d" % n)


@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
def test_pitch_canaries_nan_containment_and_graph_capture(dt):
    blk = tblock()
    F, N = 36, 24
    x, w, ws, b, val, _ = operands(F, N, 8, dt)
    kw = dict(w_self=ws, bias=b, scalers=("identity", "attenuation"), delta=DELTA, val=val, relu=True, fused=True)
    base = blk.pna(x, w, **kw)
    assert torch.isfinite(base).all().item()
    for pad, off in ((16, 4), (13, 1)):                          # pitched column views of x: narrower lanes, several column tiles per row
        xv = torch.zeros((br.NUM_X, F + pad), device=DEV, dtype=dt)[:, off:off + F]
        xv.copy_(x)
        assert not xv.is_contiguous() and same_bits(blk.pna(xv, w, **kw), base), (pad, off)
    n, guard = blk.num_dst * N, 256                              # out inside a NaN-filled buffer
    buf = torch.full((n + 2 * guard,), float("nan"), device=DEV, dtype=dt)
    out = blk.pna(x, w, out=buf[guard:guard + n].view(blk.num_dst, N), **kw)
    assert same_bits(out, base) and buf[:guard].isnan().all().item() and buf[guard + n:].isnan().all().item()
    # a NaN source row reaches, through the mean, the rows that see it and nobody else in their MFMA tile
    a = int(SB["idx"][SB["idx"] < blk.num_dst][0])               # somebody's neighbour, and the self row of destination a
    dirty = x.clone()
    dirty[int(SB["src_nodes"][a])] = float("nan")
    hit = dev(np.array([i == a or bool((SB["idx"][SB["ptr"][i]:SB["ptr"][i + 1]] == a).any()) for i in range(blk.num_dst)]))
    got = blk.pna(dirty, w, **kw)
    assert 1 < int(hit.sum()) < blk.num_dst and got[hit].isnan().all().item() and same_bits(got[~hit], base[~hit])
    # a captured launch replays to the eager bits
    x2 = operands(F, N + 1, 8, dt)[0]
    want2 = blk.pna(x2, w, **kw)
    xs, out = x.clone(), torch.full((blk.num_dst, N), 7.0, device=DEV, dtype=dt)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        blk.pna(xs, w, out=out, **kw)
    assert out.eq(7.0).all().item()                              # captured, not run
    for xin, want in ((x2, want2), (x, base), (x2, want2)):
        xs.copy_(xin)                                            # in place: the graph reads the same addresses
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want)
