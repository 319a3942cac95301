"""GPU: Block.rgcn / gnnagg_block_rgcn_run (include/gnnagg.h section F, "Block R-GCN layer") -- a typed-edge layer in one launch.
The yardsticks: for fp32 the composition of existing calls, bit for bit -- per relation r the sub-block of the edges with etype == r
(a stable filter, built here in numpy) through Block.aggregate, then relu(matmul_NN(cat([x_dst, y_0, ..], 1), cat([W_self, W_rel[0], ..], 0))
+ bias); for bf16 float64 over the stored operands (the per-relation aggregates with a bf16 out) inside the project's bf16-product bound
1e-5 * (|cat| @ |W|) (+ 2^-8 |ref| for a bf16 out).  The synthetic block has a row without edges and rows of 129 and 300 edges."""
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc

import block_run_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, B16 = torch.float32, torch.bfloat16
SB = br.synthetic_block()
PATTERNS = ("ragged", "alternating", "sorted", "random")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    view = torch.int32 if a.dtype == F32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


@functools.lru_cache(maxsize=None)
def tblock(n=SB["num_dst"]):
    """(Block on the device, its ptr in numpy): the first n rows of the synthetic block, its rows repeated where n is past them"""
    reps = -(-n // SB["num_dst"])
    deg = np.tile(np.diff(SB["ptr"]), reps)[:n]
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    e = int(ptr[-1])
    src = np.resize(SB["src_nodes"], max(br.NUM_SRC, n))
    return gnc.Block(dev(ptr), dev(np.tile(SB["idx"], reps)[:e]), dev(src), dev(np.tile(SB["eid"], reps)[:e]), n, len(src), e), ptr


@functools.lru_cache(maxsize=None)
def types(pattern, R, n=SB["num_dst"]):
    """int32 types of the block's edges (numpy).  ragged: -1 and R (outside [0, R): skipped), relation R - 1 nowhere, every third row of
    one relation only; alternating: a store / reload at every edge; sorted: one run per relation and row; random: in [0, R)."""
    ptr = tblock(n)[1]
    deg = np.diff(ptr)
    row, pos = np.repeat(np.arange(n), deg), np.arange(ptr[-1]) - np.repeat(ptr[:-1], deg)
    rng = np.random.default_rng(7 * R + n)
    if pattern == "alternating":
        t = pos % R
    elif pattern == "ragged":
        t = rng.integers(-1, R + 1, ptr[-1])
        t[t == R - 1] = R
        one = row % 3 == 0
        t[one] = (row[one] // 3) % max(R - 1, 1)
    else:
        t = rng.integers(0, R, ptr[-1])
        if pattern == "sorted":
            t = t[np.lexsort((t, row))]
    return t.astype(np.int32)


@functools.lru_cache(maxsize=None)
def sub_blocks(pattern, R, n=SB["num_dst"]):
    """per relation (the Block of its edges in CSR order, the positions kept): edges of a type outside [0, R) are in none"""
    blk, ptr = tblock(n)
    t, row = types(pattern, R, n), np.repeat(np.arange(n), np.diff(ptr))
    out = []
    for r in range(R):
        keep = np.flatnonzero(t == r)
        p = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=n))]).astype(np.int32)
        out.append((gnc.Block(dev(p), blk.idx[dev(keep)].contiguous(), blk.src_nodes, None, n, blk.num_src, len(keep)), dev(keep)))
    return out


@functools.lru_cache(maxsize=None)
def operands(F, N, R, dt, ints=False):
    """x [NUM_X, F], W_self [F, N], W_rel [R, F, N] of dt, bias [N], val per full edge: on the device, shared and never written"""
    rng = np.random.default_rng(100 * F + 10 * N + R)
    if ints:
        x, ws, wr, b = rng.integers(-4, 5, (br.NUM_X, F)), rng.integers(-1, 2, (F, N)), rng.integers(-1, 2, (R, F, N)), rng.integers(-3, 4, N)
    else:
        x, ws, wr, b = rng.standard_normal((br.NUM_X, F)), rng.standard_normal((F, N)), rng.standard_normal((R, F, N)), rng.standard_normal(N)
    f = lambda a: dev(a.astype(np.float32))
    return f(x).to(dt), f(ws).to(dt), f(wr).to(dt), f(b), f(rng.standard_normal(br.NUM_E_FULL))


def full_types(t, blk):
    """types per edge of the full CSR that give t on the block's edges (every other edge: 0, never read)"""
    full = torch.zeros(br.NUM_E_FULL, dtype=torch.int32, device=DEV)
    full[blk.eid.long()] = dev(t)
    return full


def layer(blk, pattern, x, wr, ws=None, full=False, val=None, **kw):
    """the call under test; full: types and values per edge of the full CSR, through blk.eid"""
    t = types(pattern, wr.shape[0], blk.num_dst)
    if full:
        return blk.rgcn(x, wr, full_types(t, blk), w_self=ws, etype_full=True, val=val, val_full=val is not None, **kw)
    return blk.rgcn(x, wr, dev(t), w_self=ws, val=None if val is None else val[blk.eid.long()], **kw)


def composed(blk, pattern, x, wr, ws=None, full=False, val=None, bias=None, relu=False, gathered=False, reduce="mean", fused=None, out_dtype=None):
    """the layer from the existing calls, in float64 after the aggregations: (ref, bound) with the operands' own y_r"""
    ys = [] if ws is None else [x[:blk.num_dst] if gathered else x[blk.src_nodes[:blk.num_dst].long()]]
    for sub, keep in sub_blocks(pattern, wr.shape[0], blk.num_dst):
        ys.append(sub.aggregate(x, reduce=reduce, val=None if val is None else val[blk.eid.long()][keep].contiguous(), gathered=gathered))
    cat, w = torch.cat(ys, 1), torch.cat(([] if ws is None else [ws]) + list(wr), 0)
    if x.dtype == F32:
        o = gnc.matmul_NN(cat, w)
        o = o if bias is None else o + bias
        return (torch.relu(o) if relu else o), None
    ref = cat.double() @ w.double() + (0 if bias is None else bias.double())
    return (ref.clamp_min(0) if relu else ref), 1e-5 * (cat.double().abs() @ w.double().abs()) + 1e-30


def check(out, ref, bound, what=""):
    if bound is None:
        assert same_bits(out, ref), what
        return
    err = (out.double() - ref).abs()
    if out.dtype == B16:
        bound = bound + 2.0 ** -8 * ref.abs()
    print("%s: worst |out - ref| / bound = %.4f" % (what, float((err / bound).max())))
    assert (err <= bound).all().item(), what


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("R", [1, 2, 5])
@pytest.mark.parametrize("F,N", [(1, 1), (3, 15), (20, 17), (33, 47), (128, 16), (256, 47)])
def test_fp32_is_the_composition_of_the_existing_calls_bit_for_bit(F, N, R, reduce):
    blk = tblock()[0]
    x, ws, wr, b, val = operands(F, N, R, F32)
    x_src = x[blk.src_nodes.long()].contiguous()
    everything = dict(ws=ws, bias=b, relu=True, val=val)
    variants = [everything] + [{k: v for k, v in everything.items() if k != drop} for drop in ("ws", "val", "bias")]
    variants += [dict(everything, full=True), dict(everything, gathered=True)]
    for i, v in enumerate(variants):
        xx, pattern = x_src if v.get("gathered") else x, PATTERNS[i % len(PATTERNS)]
        check(layer(blk, pattern, xx, wr, reduce=reduce, fused=True, **v), *composed(blk, pattern, xx, wr, reduce=reduce, **v),
              what="%s %s" % (pattern, sorted(v)))
    assert same_bits(layer(blk, "ragged", x, wr, reduce=reduce, fused=False, **everything), composed(blk, "ragged", x, wr, reduce=reduce, **everything)[0])


def test_one_relation_of_type_0_is_block_sage_bit_for_bit():
    blk = tblock()[0]
    x, ws, wr, b, val = operands(33, 47, 1, F32)
    v, t = val[blk.eid.long()], torch.zeros(blk.num_edges, dtype=torch.int32, device=DEV)
    for reduce in ("sum", "mean"):
        assert same_bits(blk.rgcn(x, wr, t, w_self=ws, bias=b, reduce=reduce, val=v, relu=True, fused=True),
                         blk.sage(x, wr[0], ws, b, reduce=reduce, val=v, relu=True, fused=True))


@pytest.mark.parametrize("odt", [F32, B16], ids=["out_fp32", "out_bf16"])
@pytest.mark.parametrize("F,N,R", [(1, 1, 1), (8, 8, 5), (31, 17, 2), (32, 64, 5), (100, 17, 2), (128, 64, 4)])
def test_bf16_is_inside_the_bf16_product_bound(F, N, R, odt):
    blk = tblock()[0]
    x, ws, wr, b, val = operands(F, N, R, B16)
    for i, kw in enumerate((dict(ws=ws, bias=b, val=val, reduce="mean"), dict(reduce="sum"), dict(ws=ws, reduce="sum", full=True, val=val))):
        plain = layer(blk, PATTERNS[i], x, wr, out_dtype=odt, fused=True, **kw)
        check(plain, *composed(blk, PATTERNS[i], x, wr, **kw), what="%s %s %s" % (odt, PATTERNS[i], sorted(kw)))
        assert torch.equal(layer(blk, PATTERNS[i], x, wr, out_dtype=odt, fused=True, relu=True, **kw), plain.clamp_min(0))
    # small integers, weights in {-1, 0, 1}: every product and every partial sum is exact
    x, ws, wr, b, _ = operands(F, N, R, B16, ints=True)
    ref, _ = composed(blk, "ragged", x, wr, ws=ws, bias=b, reduce="sum")
    assert torch.equal(layer(blk, "ragged", x, wr, ws=ws, bias=b, reduce="sum", out_dtype=F32, fused=True).double(), ref)


@pytest.mark.parametrize("dt,F,N", [(F32, 20, 17), (B16, 40, 24)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 15, 17, 33, "past the grid cap"])
def test_row_tile_edges_and_the_second_tile_of_a_workgroup(n, dt, F, N):
    R = 2
    if n == "past the grid cap":   # every workgroup of the capped grid takes a second tile, some a third
        cap = gnc.lib().gnnagg_block_rgcn_grid_cap(F, N, R, gnc.aggregator.FEATURE_DTYPES[dt])
        assert cap > 0
        n = 16 * (2 * cap + 3) + 5
    blk = tblock(n)[0]
    x, ws, wr, b, _ = operands(F, N, R, dt)
    out = layer(blk, "ragged", x, wr, ws=ws, bias=b, relu=True, fused=True)
    assert tuple(out.shape) == (n, N)
    check(out, *composed(blk, "ragged", x, wr, ws=ws, bias=b, relu=True), what="num_dst = %d" % n)


@pytest.mark.parametrize("dt,F,N,odt", [(F32, 100, 47, F32), (B16, 100, 64, B16)], ids=["fp32", "bf16"])
def test_pitch_canaries_and_graph_capture(dt, F, N, odt):
    blk = tblock()[0]
    x, ws, wr, b, val = operands(F, N, 3, dt)
    x2 = operands(F, N + 1, 3, dt)[0]
    t, v = dev(types("alternating", 3)), val[blk.eid.long()]
    run = lambda xx, **kw: blk.rgcn(xx, wr, t, w_self=ws, bias=b, val=v, relu=True, fused=True, **kw)
    base, base2 = run(x, out_dtype=odt), run(x2, out_dtype=odt)
    assert torch.isfinite(base).all().item()
    check(base, *composed(blk, "alternating", x, wr, ws=ws, bias=b, val=val, relu=True), what="base")
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
