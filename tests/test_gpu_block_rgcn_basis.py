"""GPU: Block.rgcn_basis / gnnagg_block_rgcn_basis_run (include/gnnagg.h section F, "Block R-GCN layer, basis decomposition").
One judge: float64 over the stored operands with the derived per-element bound of the header,
  A = |x_dst| @ |W_self| + sum_b (sum_p |comp[t_p, b]| |s_p| |x_src(p)|) @ |V_b| + |bias|,   bound = (gamma_n + 1e-5) A + 1e-30,
  gamma_n = n u / (1 - n u), u = 2^-24, n = the longest row + (B + 1) Fp + 4 (the coefficient multiply, the mean division, the chain, the
  accumulator, the bias); bf16 operands add 2^-9 (1 + gamma_n) A (the one rounding of g_b), a bf16 out 2^-8 |ref|.
The block, the type patterns and the bit comparison are those of test_gpu_block_rgcn.py."""
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc

import block_run_ref as br
from test_gpu_block_rgcn import DEV, PATTERNS, dev, full_types, same_bits, tblock, types

pytestmark = pytest.mark.gpu
F32, B16 = torch.float32, torch.bfloat16
BC = gnc.sampling.RGCN_BASIS_CHUNK[4]   # the bases of one pass at F = 20 float32: 16-byte lanes


@functools.lru_cache(maxsize=None)
def operands(F, N, R, B, dt, ints=False):
    """x [NUM_X, F], W_self [F, N], V [B, F, N] of dt, comp [R, B], bias [N], val per full edge: on the device, shared and never written"""
    rng = np.random.default_rng(1000 * F + 100 * N + 10 * R + B)
    if ints:
        x, ws, V, c, b = (rng.integers(-4, 5, (br.NUM_X, F)), rng.integers(-1, 2, (F, N)), rng.integers(-1, 2, (B, F, N)),
                          rng.integers(-1, 2, (R, B)), rng.integers(-3, 4, N))
    else:
        x, ws, V, c, b = (rng.standard_normal(s) for s in ((br.NUM_X, F), (F, N), (B, F, N), (R, B), (N,)))
    f = lambda a: dev(a.astype(np.float32))
    return f(x).to(dt), f(ws).to(dt), f(V).to(dt), f(c), f(b), f(rng.standard_normal(br.NUM_E_FULL))


def layer(blk, pattern, x, V, comp, ws=None, full=False, val=None, **kw):
    """the call under test; full: types and values per edge of the full CSR, through blk.eid"""
    t = types(pattern, comp.shape[0], blk.num_dst)
    if full:
        return blk.rgcn_basis(x, V, comp, full_types(t, blk), w_self=ws, etype_full=True, val=val, val_full=val is not None, **kw)
    return blk.rgcn_basis(x, V, comp, dev(t), w_self=ws, val=None if val is None else val[blk.eid.long()], **kw)


def judge(blk, pattern, x, V, comp, ws=None, full=False, val=None, bias=None, relu=False, gathered=False, reduce="mean"):
    """(ref, bound) in float64 over the stored operands"""
    (B, F, N), R, n = V.shape, comp.shape[0], blk.num_dst
    deg = torch.diff(blk.ptr.long())
    t = dev(types(pattern, R, n)).long()
    ok = (t >= 0) & (t < R)
    row, t = torch.repeat_interleave(torch.arange(n, device=DEV), deg)[ok], t[ok]
    s = blk.idx.long()[ok] if gathered else blk.src_nodes.long()[blk.idx.long()[ok]]
    w = torch.ones(len(t), dtype=torch.float64, device=DEV) if val is None else val[blk.eid.long()][ok].double()
    if reduce == "mean":
        cnt = torch.zeros(n * R, dtype=torch.float64, device=DEV).index_add_(0, row * R + t, torch.ones_like(w))
        w = w / cnt[row * R + t]
    xe, c = x.double()[s], comp.double()[t] * w[:, None]
    ref, A = (torch.zeros((n, N), dtype=torch.float64, device=DEV) for _ in range(2))
    for b in range(B):
        term = c[:, b, None] * xe
        ref += torch.zeros((n, F), dtype=torch.float64, device=DEV).index_add_(0, row, term) @ V[b].double()
        A += torch.zeros((n, F), dtype=torch.float64, device=DEV).index_add_(0, row, term.abs()) @ V[b].double().abs()
    if ws is not None:
        xd = x.double()[:n] if gathered else x.double()[blk.src_nodes[:n].long()]
        ref, A = ref + xd @ ws.double(), A + xd.abs() @ ws.double().abs()
    if bias is not None:
        ref, A = ref + bias.double(), A + bias.double().abs()
    Fp = -(-F // 32) * 32 if x.dtype == B16 else -(-F // 4) * 4
    nu = (int(deg.max()) + (B + 1) * Fp + 4) * 2.0 ** -24
    gamma = nu / (1 - nu)
    bound = (gamma + 1e-5) * A + 1e-30
    if x.dtype == B16:
        bound = bound + 2.0 ** -9 * (1 + gamma) * A
    return (ref.clamp_min(0) if relu else ref), bound


def check(out, ref, bound, what=""):
    err = (out.double() - ref).abs()
    if out.dtype == B16:
        bound = bound + 2.0 ** -8 * ref.abs()
    print("%s: worst |out - ref| / bound = %.4f" % (what, float((err / bound).max())))
    assert (err <= bound).all().item(), what


FP32_SHAPES = [(1, 1, 1, 1), (3, 15, 5, 2), (33, 47, 2, 5), (20, 17, 200, BC), (20, 17, 200, BC + 1), (128, 16, 266, 8), (256, 47, 40, 4)]
BF16_SHAPES = [(1, 1, 1, 1), (31, 17, 5, 2), (64, 64, 200, 8), (128, 64, 46, 4)]
CASES = [(F32, F32) + s for s in FP32_SHAPES] + [(B16, odt) + s for s in BF16_SHAPES for odt in (F32, B16)]


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("dt,odt,F,N,R,B", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_inside_the_float64_bound(dt, odt, F, N, R, B, reduce):
    blk = tblock()[0]
    x, ws, V, comp, b, val = operands(F, N, R, B, dt)
    x_src = x[blk.src_nodes.long()].contiguous()
    everything = dict(ws=ws, bias=b, relu=True, val=val)
    variants = [everything] + [{k: v for k, v in everything.items() if k != drop} for drop in ("ws", "val", "bias")]
    variants += [dict(everything, full=True), dict(everything, gathered=True)]
    for i, v in enumerate(variants):
        xx, pattern = x_src if v.get("gathered") else x, PATTERNS[i % len(PATTERNS)]
        check(layer(blk, pattern, xx, V, comp, reduce=reduce, out_dtype=odt, fused=True, **v), *judge(blk, pattern, xx, V, comp, reduce=reduce, **v),
              what="%s %s" % (pattern, sorted(v)))
    if (F, N, R, B) == (33, 47, 2, 5):   # the composition: its chains and its product are no longer than the kernel's here (R < B)
        check(layer(blk, "ragged", x, V, comp, reduce=reduce, fused=False, **everything), *judge(blk, "ragged", x, V, comp, reduce=reduce, **everything),
              what="fused=False")


@pytest.mark.parametrize("R", [1, 2, 5])
@pytest.mark.parametrize("F,N", [(3, 15), (20, 17), (128, 16)])
def test_identity_comp_is_block_rgcn_bit_for_bit(F, N, R):
    blk = tblock()[0]
    x, ws, V, _, b, val = operands(F, N, R, R, F32)
    eye, v = torch.eye(R, device=DEV), val[blk.eid.long()]
    for pattern in PATTERNS:
        t = dev(types(pattern, R))
        kw = dict(w_self=ws, bias=b, reduce="sum", val=v, relu=True, fused=True)
        assert same_bits(blk.rgcn_basis(x, V, eye, t, **kw), blk.rgcn(x, V, t, **kw)), pattern


@pytest.mark.parametrize("dt,F,N,R,B", [(F32, 20, 17, 5, 3), (F32, 33, 47, 200, BC + 1), (B16, 31, 17, 5, 2), (B16, 64, 64, 200, 8)])
def test_small_integers_are_exact(dt, F, N, R, B):
    blk = tblock()[0]
    x, ws, V, comp, b, _ = operands(F, N, R, B, dt, ints=True)
    out = layer(blk, "ragged", x, V, comp, ws=ws, bias=b, reduce="sum", out_dtype=F32, fused=True)
    assert torch.equal(out.double(), judge(blk, "ragged", x, V, comp, ws=ws, bias=b, reduce="sum")[0])


@pytest.mark.parametrize("dt,F,N,B", [(F32, 20, 17, 2), (B16, 40, 24, 3)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 15, 17, 33, "past the grid cap"])
def test_row_tile_edges_and_the_count_table_of_the_next_tile(n, dt, F, N, B):
    R = 200
    if n == "past the grid cap":   # every workgroup of the capped grid takes a second tile, some a third
        cap = gnc.lib().gnnagg_block_rgcn_basis_grid_cap(F, N, R, B, gnc.aggregator.FEATURE_DTYPES[dt])
        assert cap > 0
        n = 16 * (2 * cap + 3) + 5
    blk = tblock(n)[0]
    x, ws, V, comp, b, _ = operands(F, N, R, B, dt)
    out = layer(blk, "ragged", x, V, comp, ws=ws, bias=b, relu=True, fused=True)
    assert tuple(out.shape) == (n, N)
    check(out, *judge(blk, "ragged", x, V, comp, ws=ws, bias=b, relu=True), what="num_dst = %d" % n)


@pytest.mark.parametrize("dt,F,N,odt", [(F32, 100, 47, F32), (B16, 100, 64, B16)], ids=["fp32", "bf16"])
def test_pitch_canaries_and_graph_capture(dt, F, N, odt):
    blk = tblock()[0]
    x, ws, V, comp, b, val = operands(F, N, 40, 3, dt)
    x2 = operands(F, N + 1, 40, 3, dt)[0]
    t, v = dev(types("alternating", 40)), val[blk.eid.long()]
    run = lambda xx, **kw: blk.rgcn_basis(xx, V, comp, t, w_self=ws, bias=b, val=v, relu=True, fused=True, **kw)
    base, base2 = run(x, out_dtype=odt), run(x2, out_dtype=odt)
    assert torch.isfinite(base).all().item()
    check(base, *judge(blk, "alternating", x, V, comp, ws=ws, bias=b, val=val, relu=True), what="base")
    for pad, off in ((16, 4), (13, 1)):    # a pitched column view: 16-byte lanes, and one-element lanes over several column tiles
        wide = torch.zeros((br.NUM_X, F + pad), device=DEV, dtype=dt)
        xv = wide[:, off:off + F]
        xv.copy_(x)
        assert not xv.is_contiguous() and same_bits(run(xv, out_dtype=odt), base), (pad, off)
    n, guard = blk.num_dst * N, 256
    buf = torch.full((n + 2 * guard,), float("nan"), device=DEV, dtype=odt)
    out = buf[guard:guard + n].view(blk.num_dst, N)
    xs = x.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(xs, out=out)
    assert out.isnan().all().item()                          # captured, not run
    for xin, want in ((x2, base2), (x, base), (x2, base2)):
        xs.copy_(xin)                                        # in place: the graph reads the same addresses
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want) and buf[:guard].isnan().all().item() and buf[guard + n:].isnan().all().item()
