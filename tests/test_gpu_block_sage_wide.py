"""GPU: Block.sage(fused="wide") / gnnagg_block_sage_wide_run (include/gnnagg.h section F, "Block SAGE layer, wide rows") -- the SAGE layer
in one launch for rows up to 4096 features, k in chunks of KC = gnnagg_block_sage_wide_chunk(dtype) columns.  The yardsticks are those of
test_gpu_block_sage.py: fp32 the composition aggregate + matmul_NN bit for bit; bf16 float64 over the stored operands inside
1e-5 * (|cat| @ |W|) (+ 2^-8 |ref| for a bf16 out); and, where both kernels serve a shape, the narrow kernel's bits.  A feat is written
(a, b) = a * KC + b, resolved inside the test."""
import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc

import block_run_ref as br
from test_gpu_block_sage import B16, DEV, F32, SB, check, composed, dev, offset_copy, operands, same_bits, tblock

pytestmark = pytest.mark.gpu
TILE_ROWS = {F32: 16, B16: 64}    # rows of a workgroup's tile: 16 R, R = 4 for bf16 with n_out <= 128


def kc(dt):
    return gnc.lib().gnnagg_block_sage_wide_chunk(gnc.aggregator.FEATURE_DTYPES[dt])


def feat_of(ab, dt):
    return ab[0] * kc(dt) + ab[1]


def wide(blk, x, wn, ws=None, **kw):
    return blk.sage(x, wn, w_self=ws, fused="wide", **kw)


FEATS_F32 = [(0, 1), (0, 3), (1, -1), (1, 0), (1, 1), (0, 257), (2, 4), (0, 602)]


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("ab,N", [(ab, n) for ab in FEATS_F32 for n in (1, 17, 64, 256)] + [((0, 4096), 17)])
def test_fp32_is_the_composition_of_the_existing_calls_bit_for_bit(ab, N, reduce):
    blk, F = tblock(), feat_of(ab, F32)
    x, ws, wn, b, val, full = operands(F, N, F32)
    x_src = x[blk.src_nodes.long()].contiguous()
    everything = dict(ws=ws, bias=b, relu=True, val=val)
    variants = [everything] + [{k: v for k, v in everything.items() if k != drop} for drop in ("ws", "bias")]
    variants += [dict(everything, val=full, val_full=True), dict(everything, gathered=True)]
    for v in variants:
        xx = x_src if v.get("gathered") else x
        out = wide(blk, xx, wn, reduce=reduce, **v)
        check(out, *composed(blk, xx, wn, reduce=reduce, **v), what=str(sorted(v)))
        if gnc.block_sage_supported(F, N, F32):
            assert same_bits(out, blk.sage(xx, wn, w_self=v.get("ws"), fused=True, reduce=reduce, **{k: a for k, a in v.items() if k != "ws"}))


@pytest.mark.parametrize("odt", [F32, B16], ids=["out_fp32", "out_bf16"])
@pytest.mark.parametrize("ab", [(1, -1), (1, 1), (0, 257), (0, 602), (0, 1024)])
@pytest.mark.parametrize("N", [17, 128, 256])
def test_bf16_is_inside_the_bf16_product_bound(ab, N, odt):
    blk, F = tblock(), feat_of(ab, B16)
    x, ws, wn, b, val, _ = operands(F, N, B16)
    for kw in (dict(ws=ws, bias=b, val=val, reduce="mean"), dict(reduce="sum"), dict(ws=ws, reduce="max")):
        plain = wide(blk, x, wn, out_dtype=odt, **kw)
        check(plain, *composed(blk, x, wn, out_dtype=B16, **kw), what="%s %s" % (odt, sorted(kw)))
        assert torch.equal(wide(blk, x, wn, out_dtype=odt, relu=True, **kw), plain.clamp_min(0))
        if gnc.block_sage_supported(F, N, B16):   # the same tile rounding, the same MFMA k blocks in the same order: the narrow kernel's bits
            assert same_bits(plain, blk.sage(x, wn, w_self=kw.get("ws"), fused=True, out_dtype=odt, **{k: a for k, a in kw.items() if k != "ws"}))
    # small integers, weights in {-1, 0, 1}: every product and every partial sum is exact
    x, ws, wn, b, _, _ = operands(F, N, B16, ints=True)
    ref, _ = composed(blk, x, wn, ws=ws, bias=b, reduce="sum", out_dtype=B16)
    assert torch.equal(blk.sage(x, wn, ws, b, reduce="sum", out_dtype=F32, fused="wide").double(), ref)


@pytest.mark.parametrize("dt,N", [(F32, 17), (B16, 24)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 65, "past the grid cap"])
def test_row_tile_edges_and_the_second_tile_of_a_workgroup(n, dt, N):
    F = 2 * kc(dt) + 4
    if n == "past the grid cap":   # every workgroup of the capped grid takes a second tile, some a third
        cap = gnc.lib().gnnagg_block_sage_wide_grid_cap(F, N, gnc.aggregator.FEATURE_DTYPES[dt])
        assert cap > 0
        n = TILE_ROWS[dt] * (2 * cap + 3) + 5
    blk = tblock(n)
    x, ws, wn, b, _, _ = operands(F, N, dt)
    out = blk.sage(x, wn, ws, b, reduce="mean", relu=True, fused="wide")
    assert tuple(out.shape) == (n, N)
    check(out, *composed(blk, x, wn, ws=ws, bias=b, relu=True, reduce="mean"), what="num_dst = %d" % n)


@pytest.mark.parametrize("dt,N,odt", [(F32, 47, F32), (B16, 64, B16), (B16, 17, F32)], ids=["fp32", "bf16", "bf16_out_fp32"])
def test_alignment_pitch_canaries_and_a_nan_row(dt, N, odt):
    blk, F = tblock(), 2 * kc(dt) + 4
    x, ws, wn, b, val, _ = operands(F, N, dt)
    kw = dict(bias=b, reduce="mean", val=val, relu=True, fused="wide")
    base = blk.sage(x, wn, ws, out_dtype=odt, **kw)
    assert torch.isfinite(base).all().item()
    for pad, off in ((16, 0), (16, 4), (13, 2), (13, 1)):    # lanes of every width down to one element: several column tiles inside a chunk
        wide_x = torch.zeros((br.NUM_X, F + pad), device=DEV, dtype=dt)
        xv = wide_x[:, off:off + F]
        xv.copy_(x)
        assert not xv.is_contiguous() and same_bits(blk.sage(xv, wn, ws, out_dtype=odt, **kw), base), (pad, off)
    n, guard = blk.num_dst * N, 256
    for off in (0, 1, 2, 4):    # weights off 16-byte alignment (bf16: the 2-byte staging); out anywhere inside a NaN-filled buffer
        buf = torch.full((n + 2 * guard,), float("nan"), device=DEV, dtype=odt)
        out = blk.sage(x, offset_copy(wn, off), offset_copy(ws, off), out=buf[guard + off:guard + off + n].view(blk.num_dst, N), **kw)
        assert same_bits(out, base) and buf[:guard + off].isnan().all().item() and buf[guard + off + n:].isnan().all().item(), off
    # a NaN source row reaches its neighbours and itself, in every column, and nobody else
    a = int(SB["idx"][SB["idx"] < blk.num_dst][0])
    dirty = x.clone()
    dirty[int(SB["src_nodes"][a])] = float("nan")
    hit = dev(np.array([i == a or bool((SB["idx"][SB["ptr"][i]:SB["ptr"][i + 1]] == a).any()) for i in range(blk.num_dst)]))
    assert 1 < int(hit.sum()) < blk.num_dst
    out = blk.sage(dirty, wn, ws, out_dtype=odt, **kw)
    assert out[hit].isnan().all().item() and same_bits(out[~hit], base[~hit])


@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
def test_side_stream_and_graph_capture(dt):
    blk = tblock()
    F, N = 602, 24
    x1, ws, wn, b, val, _ = operands(F, N, dt)
    x2 = operands(F, N + 1, dt)[0]
    kw = dict(bias=b, reduce="mean", val=val, relu=True, fused="wide")
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
