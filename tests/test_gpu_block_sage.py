"""GPU: Block.sage / gnnagg_block_sage_run (include/gnnagg.h section F, "Block SAGE layer") -- one launch per layer of a sampled block.
The yardsticks: for fp32 the composition of existing calls, relu(matmul_NN(cat([x_dst, y]), cat([W_self, W_neigh])) + bias) with
y, x_dst = blk.aggregate(..., return_dst=True), bit for bit; for bf16 float64 over the stored operands inside the project's bf16-product
bound 1e-5 * (|cat| @ |W|) (+ 2^-8 |ref| for a bf16 out: one rounding, at most 2^-9 relative, doubled for a tie at the boundary)."""
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc

import block_run_ref as br
import sampling_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, B16 = torch.float32, torch.bfloat16
SB = br.synthetic_block()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    view = torch.int32 if a.dtype == F32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


@functools.lru_cache(maxsize=None)
def tblock(n=SB["num_dst"]):
    """the first n rows of the synthetic block, its rows repeated where n is past them; src_nodes repeated with them (the self rows)"""
    reps = -(-n // SB["num_dst"])
    deg = np.tile(np.diff(SB["ptr"]), reps)[:n]
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    e = int(ptr[-1])
    src = np.resize(SB["src_nodes"], max(br.NUM_SRC, n))
    return gnc.Block(dev(ptr), dev(np.tile(SB["idx"], reps)[:e]), dev(src), dev(np.tile(SB["eid"], reps)[:e]), n, len(src), e)


@functools.lru_cache(maxsize=None)
def operands(F, N, dt, ints=False):
    """x [NUM_X, F], W_self, W_neigh [F, N] of dt, bias [N], val per block edge and per full edge: on the device, shared and never written"""
    rng = np.random.default_rng(100 * F + N)
    if ints:
        x, ws, wn, b = rng.integers(-4, 5, (br.NUM_X, F)), rng.integers(-1, 2, (F, N)), rng.integers(-1, 2, (F, N)), rng.integers(-3, 4, N)
    else:
        x, ws, wn, b = rng.standard_normal((br.NUM_X, F)), rng.standard_normal((F, N)), rng.standard_normal((F, N)), rng.standard_normal(N)
    full = rng.standard_normal(br.NUM_E_FULL).astype(np.float32)
    f = lambda a: dev(a.astype(np.float32))
    return f(x).to(dt), f(ws).to(dt), f(wn).to(dt), f(b), dev(full[SB["eid"]]), dev(full)


def fused(blk, x, wn, ws=None, **kw):
    return blk.sage(x, wn, w_self=ws, fused=True, **kw)


def composed(blk, x, wn, ws=None, bias=None, relu=False, gathered=False, **kw):
    """the layer from the existing calls, in float64 after the aggregation: (ref, bound) with the operands' own y"""
    if gathered:
        y, x_dst = blk.aggregate(x, gathered=True, **kw), x[:blk.num_dst]
    else:
        y, x_dst = blk.aggregate(x, return_dst=True, **kw)
    cat, w = (y, wn) if ws is None else (torch.cat([x_dst, y], 1), torch.cat([ws, wn], 0))
    if x.dtype == F32:
        o = gnc.matmul_NN(cat.contiguous(), w.contiguous())
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


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("F,N", [(1, 1), (3, 15), (4, 16), (20, 17), (33, 47), (100, 128), (128, 16), (256, 47)])
def test_fp32_is_the_composition_of_the_existing_calls_bit_for_bit(F, N, reduce):
    blk = tblock()
    x, ws, wn, b, val, full = operands(F, N, F32)
    x_src = x[blk.src_nodes.long()].contiguous()
    everything = dict(ws=ws, bias=b, relu=True, val=val)
    variants = [everything] + [{k: v for k, v in everything.items() if k != drop} for drop in everything]
    variants += [dict(everything, val=full, val_full=True), dict(everything, gathered=True)]
    for v in variants:
        xx = x_src if v.get("gathered") else x
        check(fused(blk, xx, wn, reduce=reduce, **v), *composed(blk, xx, wn, reduce=reduce, **v), what=str(sorted(v)))
    assert same_bits(gnc.block_sage_run(blk, x, wn, w_self=ws, bias=b, reduce=reduce), blk.sage(x, wn, ws, b, reduce=reduce, fused=False))


@pytest.mark.parametrize("odt", [F32, B16], ids=["out_fp32", "out_bf16"])
@pytest.mark.parametrize("F,N", [(1, 1), (8, 8), (31, 17), (32, 64), (33, 128), (100, 17), (128, 128)])
def test_bf16_is_inside_the_bf16_product_bound(F, N, odt):
    blk = tblock()
    x, ws, wn, b, val, _ = operands(F, N, B16)
    for kw in (dict(ws=ws, bias=b, val=val, reduce="mean"), dict(reduce="sum"), dict(ws=ws, reduce="max")):
        plain = fused(blk, x, wn, out_dtype=odt, **kw)
        check(plain, *composed(blk, x, wn, out_dtype=B16, **kw), what="%s %s" % (odt, sorted(kw)))
        assert torch.equal(fused(blk, x, wn, out_dtype=odt, relu=True, **kw), plain.clamp_min(0))
    # small integers, weights in {-1, 0, 1}: every product and every partial sum is exact
    x, ws, wn, b, _, _ = operands(F, N, B16, ints=True)
    ref, _ = composed(blk, x, wn, ws=ws, bias=b, reduce="sum", out_dtype=B16)
    assert torch.equal(blk.sage(x, wn, ws, b, reduce="sum", out_dtype=F32, fused=True).double(), ref)


@pytest.mark.parametrize("dt,F,N", [(F32, 20, 17), (B16, 40, 24)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, "past the grid cap"])
def test_row_tile_edges_and_the_second_tile_of_a_workgroup(n, dt, F, N):
    if n == "past the grid cap":   # every workgroup of the capped grid takes a second tile, some a third
        cap = gnc.lib().gnnagg_block_sage_grid_cap(F, N, gnc.aggregator.FEATURE_DTYPES[dt])
        assert cap > 0
        n = 16 * (2 * cap + 3) + 5
    blk = tblock(n)
    x, ws, wn, b, _, _ = operands(F, N, dt)
    out = blk.sage(x, wn, ws, b, reduce="mean", relu=True, fused=True)
    assert tuple(out.shape) == (n, N)
    check(out, *composed(blk, x, wn, ws=ws, bias=b, relu=True, reduce="mean"), what="num_dst = %d" % n)


def offset_copy(t, off):
    """a dense copy of t that starts `off` elements into a 64-byte aligned allocation"""
    flat = torch.zeros(t.numel() + 16, device=DEV, dtype=t.dtype)
    return flat[off:off + t.numel()].view(t.shape).copy_(t)


@pytest.mark.parametrize("dt,F,N,odt", [(F32, 100, 47, F32), (B16, 100, 64, B16), (B16, 33, 17, F32)], ids=["fp32", "bf16", "bf16_out_fp32"])
def test_alignment_pitch_and_canaries(dt, F, N, odt):
    blk = tblock()
    x, ws, wn, b, val, _ = operands(F, N, dt)
    kw = dict(bias=b, reduce="mean", val=val, relu=True, fused=True)
    base = blk.sage(x, wn, ws, out_dtype=odt, **kw)
    assert torch.isfinite(base).all().item()
    for pad, off in ((16, 0), (16, 4), (13, 2), (13, 1)):    # lanes of every width down to one element; pitch 13: several column tiles per row
        wide = torch.zeros((br.NUM_X, F + pad), device=DEV, dtype=dt)
        xv = wide[:, off:off + F]
        xv.copy_(x)
        assert not xv.is_contiguous() and same_bits(blk.sage(xv, wn, ws, out_dtype=odt, **kw), base), (pad, off)
    n, guard = blk.num_dst * N, 256
    for off in (0, 1, 2, 4):    # weights off 16-byte alignment (bf16: the 2-byte staging); out anywhere inside a NaN-filled buffer
        buf = torch.full((n + 2 * guard,), float("nan"), device=DEV, dtype=odt)
        out = blk.sage(x, offset_copy(wn, off), offset_copy(ws, off), out=buf[guard + off:guard + off + n].view(blk.num_dst, N), **kw)
        assert same_bits(out, base) and buf[:guard + off].isnan().all().item() and buf[guard + off + n:].isnan().all().item(), off


@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
def test_a_nan_row_reaches_its_neighbours_and_itself_only(dt):
    blk = tblock()
    F, N = 20, 17
    clean, ws, wn, b, val, _ = operands(F, N, dt)
    a = int(SB["idx"][SB["idx"] < blk.num_dst][0])           # a source row that is somebody's neighbour, and the self row of destination a
    dirty = clean.clone()
    dirty[int(SB["src_nodes"][a])] = float("nan")
    hit = np.array([i == a or bool((SB["idx"][SB["ptr"][i]:SB["ptr"][i + 1]] == a).any()) for i in range(blk.num_dst)])
    assert hit.sum() > 1 and not hit.all()
    hit_t = dev(hit)
    for reduce in ("sum", "mean"):
        kw = dict(bias=b, reduce=reduce, val=val, relu=True, fused=True)
        out, want = blk.sage(dirty, wn, ws, **kw), blk.sage(clean, wn, ws, **kw)
        assert out[hit_t].isnan().all().item(), reduce       # every column: no garbage in the tile's padding, ReLU keeps a NaN
        assert same_bits(out[~hit_t], want[~hit_t]), reduce  # and nobody else: no leak across the rows of an MFMA tile


@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
def test_side_stream_and_graph_capture(dt):
    blk = tblock()
    F, N = 36, 24
    x1, ws, wn, b, val, _ = operands(F, N, dt)
    x2 = operands(F, N + 1, dt)[0]
    kw = dict(bias=b, reduce="mean", val=val, relu=True, fused=True)
    want1, want2 = blk.sage(x1, wn, ws, **kw), blk.sage(x2, wn, ws, **kw)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        got = blk.sage(x1, wn, ws, **kw)
    torch.cuda.synchronize()
    assert same_bits(got, want1)
    xs, out = x1.clone(), torch.full((blk.num_dst, N), 7.0, device=DEV, dtype=dt)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        blk.sage(xs, wn, ws, out=out, **kw)
    assert out.eq(7.0).all().item()                          # captured, not run
    for xin, want in ((x2, want2), (x1, want1), (x2, want2)):
        xs.copy_(xin)                                        # in place: the graph reads the same addresses
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want)


@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
def test_a_two_layer_sampled_batch(dt):
    ptr, idx = (dev(a) for a in sr.fixture_graph())
    V, dims = ptr.numel() - 1, (32, 48, 17)
    rng = np.random.default_rng(5)
    h = dev(rng.standard_normal((V, dims[0])).astype(np.float32)).to(dt)
    seeds = dev(np.concatenate([sr.crafted_rows(), rng.choice(V, 200, replace=False)]).astype(np.int32))
    sampler = gnc.NeighborSampler(ptr, idx)
    blocks = sampler.sample_layers(seeds, fanouts=(5, 5), seed=20)
    sampler.close()
    h_c = h
    for l, blk in enumerate(blocks):
        ws, wn = (dev(rng.standard_normal((dims[l], dims[l + 1])).astype(np.float32)).to(dt) for _ in range(2))
        b = dev(rng.standard_normal(dims[l + 1]).astype(np.float32))
        kw = dict(bias=b, reduce="mean", relu=l == 0, gathered=l > 0)
        out = blk.sage(h, wn, ws, fused=True, **kw)
        check(out, *composed(blk, h, wn, ws=ws, **kw), what="layer %d" % l)       # bf16: float64 over what this layer was given
        h_c = blk.sage(h_c, wn, ws, fused=False, **kw)
        h = out
    assert tuple(h.shape) == (seeds.numel(), dims[2]) and h_c.dtype == h.dtype
    if dt == F32:
        assert same_bits(h, h_c)                             # the whole batch: the composition's bits
