"""GPU: gnc.pair_score / Block.score / gnnagg_pair_score_run (include/gnnagg.h section G, "Pair scoring").
The yardsticks: float64 over the stored operands for dot, DistMult and the bf16 mlp; the composition of existing calls
(pair_score(fused=False)), bit for bit, for the fp32 mlp; the COO form, bit for bit, for the CSR form.
dot: |out - ref| <= (gamma_n + 1e-5) A + 1e-30 with A = sum_f |hu| |rel| |hv|, n = roundup32(F) + 8, gamma_n = n u / (1 - n u), u = 2^-24 -- a
lane's chain and the butterfly are at most n fp32 roundings per term (DistMult's extra product is one of them); bf16 products are exact
in fp32, so both dtypes share it; 1e-5 is the project's slack.
bf16 mlp: the bound of tests/test_gpu_block_gin.py without the chain term: A_1 = |m| |W1| + |b1|, A_2 = A_1 |W2| + |b2|, u16 = 2^-8,
|out - ref| <= ((1 + gamma_n)(1 + u16)^2 - 1 + 1e-5) A_2 + 1e-30 with n = Kp + Hp + 8 (Kp: the padded k of W1) -- the two bf16 roundings of m
and z -- and a bf16 out adds u16 (|ref| + bound).
Measured on one MI355X: the worst |out - ref| / bound of this file is 0.0086 for dot / DistMult (F = 3, fp32) and 0.741 for the bf16 mlp
(mul 1 -> 1 -> 1, no biases, a fp32 out; 0.014 and less at 128 -> 128 -> 1)."""
import functools

import numpy as np
import pytest
import torch

import gnn_computing_amd as gnc
from gnn_computing_amd import _lib

from test_gpu_block_sage import B16, DEV, F32, dev, same_bits, tblock

pytestmark = pytest.mark.gpu
NODES, NREL = 300, 5
DEG = [0, 0, 3, 0, 0, 0, 70, 1, 0, 2, 16, 0, 0]   # empty rows first, last and in runs; a row longer than a 64-lane group's window


@functools.lru_cache(maxsize=None)
def operands(F, H, N, dt, cat=False, ints=False, rows=NODES):
    """hu, hv [rows, F], W1 [F or 2 F, H], W2 [H, N] of dt, b1, b2, rel [NREL, F]: on the device, shared and never written"""
    rng = np.random.default_rng(10000 * F + 100 * H + N)
    draw = (lambda lo, hi, s: rng.integers(lo, hi + 1, s)) if ints else (lambda lo, hi, s: rng.standard_normal(s))
    f = lambda a: dev(a.astype(np.float32))
    hu, hv, w1, w2 = draw(-4, 4, (rows, F)), draw(-4, 4, (rows, F)), draw(-1, 1, ((2 if cat else 1) * F, max(H, 1))), draw(-1, 1, (max(H, 1), max(N, 1)))
    return f(hu).to(dt), f(hv).to(dt), f(w1).to(dt), f(w2).to(dt), f(draw(-3, 3, max(H, 1))), f(draw(-3, 3, max(N, 1))), f(draw(-2, 2, (NREL, F)))


@functools.lru_cache(maxsize=None)
def coo_pairs():
    """90 pairs with a run of equal u, u == v, repeated pairs; types that include -1 and NREL"""
    rng = np.random.default_rng(3)
    u, v, t = rng.integers(0, NODES, 90), rng.integers(0, NODES, 90), rng.integers(0, NREL, 90)
    u[10:31] = 17
    v[40:45] = u[40:45]
    u[50:53], v[50:53] = u[47:50], v[47:50]
    t[[3, 60]], t[[12, 89]] = -1, NREL
    return tuple(dev(a.astype(np.int32)) for a in (u, v, t))


def check_bound(out, ref, bound, what):
    if out.dtype == B16:
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)
    err = (out.double() - ref).abs()
    print("%s: worst |out - ref| / bound = %.4f" % (what, float((err / bound).max())))
    assert (err <= bound).all().item(), what


@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("F", [1, 3, 4, 20, 33, 100, 256])
def test_dot_and_distmult_against_float64(F, dt):
    u, v, t = coo_pairs()
    nu = (-(-F // 32) * 32 + 8) * 2.0 ** -24
    for ints in (False, True):
        hu, hv, _, _, _, _, rel = operands(F, 0, 0, dt, ints=ints)
        a, b = hu.double()[u.long()], hv.double()[v.long()]
        ok = ((t >= 0) & (t < NREL))[:, None]
        r = torch.where(ok, rel.double()[t.clamp(0, NREL - 1).long()], torch.zeros((), device=DEV, dtype=torch.float64))
        for what, out, terms in (("dot", gnc.pair_score(hu, hv, u=u, v=v), a * b), ("distmult", gnc.pair_score(hu, hv, u=u, v=v, rel=rel, etype=t), a * r * b)):
            assert out.dtype == F32 and tuple(out.shape) == (90,)
            if ints:
                assert torch.equal(out.double(), terms.sum(1)), what
            else:
                check_bound(out, terms.sum(1), (nu / (1 - nu) + 1e-5) * terms.abs().sum(1) + 1e-30, "%s F = %d %s" % (what, F, dt))


@pytest.mark.parametrize("P", [1, 15, 16, 17, 33, "past the grid cap"])
def test_csr_form_equals_coo_form_bit_for_bit(P):
    F, H, N = 20, 17, 33
    if P == "past the grid cap":   # every workgroup of the capped mlp grid takes a second tile, some a third (tiles of at most 64 pairs)
        cap = gnc.lib().gnnagg_pair_score_grid_cap(_lib.PAIR_MLP, _lib.PAIR_MUL, F, H, N, _lib.DTYPE_F32)
        assert 0 < cap < 2 ** 20
        P = 64 * (2 * cap + 3) + 5
    reps = -(-P // sum(DEG)) + 1
    deg = np.tile(DEG, reps)
    n = len(deg)
    ptr = np.minimum(np.concatenate([[0], np.cumsum(deg)]), P).astype(np.int32)     # the first P positions: every later row is empty
    rng = np.random.default_rng(P)
    idx, src = rng.integers(0, n, P).astype(np.int32), rng.integers(0, n, n).astype(np.int32)
    urow = np.repeat(np.arange(n), np.diff(ptr)).astype(np.int32)
    ptr, idx, src, urow = dev(ptr), dev(idx), dev(src), dev(urow)
    etype = dev(rng.integers(-1, NREL + 1, P).astype(np.int32))
    for dt in (F32, B16):
        hu, hv, w1, w2, b1, b2, rel = operands(F, H, N, dt, rows=n)
        wide = torch.zeros((n, F + 13), device=DEV, dtype=dt)
        wide[:, 1:1 + F] = hu
        for kw in (dict(kind="dot"), dict(kind="dot", rel=rel, etype=etype), dict(kind="mlp", w1=w1, w2=w2, b1=b1, b2=b2, relu=True, fused=True)):
            for s in (None, src):
                for h in (hu, wide[:, 1:1 + F]):
                    got = gnc.pair_score(h, hv, ptr=ptr, idx=idx, src=s, **kw)
                    assert same_bits(got, gnc.pair_score(h, hv, u=urow, v=idx, src=s, **kw)), (P, dt, sorted(kw), s is not None, h is hu)


@pytest.mark.parametrize("combine", ["mul", "cat"])
@pytest.mark.parametrize("F,H,N", [(1, 1, 1), (3, 5, 1), (4, 16, 16), (20, 17, 33), (33, 47, 1), (100, 128, 47), (256, 256, 1)])
def test_mlp_fp32_is_the_composition_of_the_existing_calls_bit_for_bit(F, H, N, combine):
    u, v, _ = coo_pairs()
    hu, hv, w1, w2, b1, b2, _ = operands(F, H, N, F32, cat=combine == "cat")
    everything = dict(b1=b1, b2=b2, relu=True)
    for kw in [everything] + [{k: x for k, x in everything.items() if k != drop} for drop in everything]:
        fused = gnc.pair_score(hu, hv, u=u, v=v, kind="mlp", combine=combine, w1=w1, w2=w2, fused=True, **kw)
        assert tuple(fused.shape) == (90, N)
        assert same_bits(fused, gnc.pair_score(hu, hv, u=u, v=v, kind="mlp", combine=combine, w1=w1, w2=w2, fused=False, **kw)), sorted(kw)


@pytest.mark.parametrize("odt", [F32, B16], ids=["out_fp32", "out_bf16"])
@pytest.mark.parametrize("combine", ["mul", "cat"])
@pytest.mark.parametrize("F,H,N", [(1, 1, 1), (8, 8, 1), (31, 33, 17), (32, 64, 64), (128, 128, 1)])
def test_mlp_bf16_is_inside_the_derived_float64_bound(F, H, N, combine, odt):
    u, v, _ = coo_pairs()
    hu, hv, w1, w2, b1, b2, _ = operands(F, H, N, B16, cat=combine == "cat")
    a, b = hu.double()[u.long()], hv.double()[v.long()]
    m = torch.cat([a, b], 1) if combine == "cat" else a * b
    nu = (-(-m.shape[1] // 32) * 32 + -(-H // 32) * 32 + 8) * 2.0 ** -24
    for kw in (dict(b1=b1, b2=b2), dict()):
        b1d, b2d = (kw["b1"].double(), kw["b2"].double()) if kw else (0.0, 0.0)
        ref = (m @ w1.double() + b1d).clamp_min(0) @ w2.double() + b2d
        a_2 = (m.abs() @ w1.double().abs() + abs(b1d)) @ w2.double().abs() + abs(b2d)
        bound = ((1 + nu / (1 - nu)) * (1 + 2.0 ** -8) ** 2 - 1 + 1e-5) * a_2 + 1e-30
        plain = gnc.pair_score(hu, hv, u=u, v=v, kind="mlp", combine=combine, w1=w1, w2=w2, out_dtype=odt, fused=True, **kw)
        check_bound(plain, ref, bound, "%s %s %s" % (combine, odt, sorted(kw)))
        relu = gnc.pair_score(hu, hv, u=u, v=v, kind="mlp", combine=combine, w1=w1, w2=w2, out_dtype=odt, fused=True, relu=True, **kw)
        assert torch.equal(relu, plain.clamp_min(0))


@pytest.mark.parametrize("dt", [F32, B16], ids=["fp32", "bf16"])
def test_block_score_is_pair_score_over_the_blocks_arrays(dt):
    blk = tblock()
    F, H, N = 36, 20, 3
    hd, hs, w1, w2, b1, b2, rel = operands(F, H, N, dt, cat=True, rows=1000)
    etype = dev((np.arange(blk.num_edges) % (NREL + 2) - 1).astype(np.int32))
    for kw in (dict(), dict(rel=rel, etype=etype), dict(kind="mlp", combine="cat", w1=w1, w2=w2, b1=b1, fused=True)):
        want = gnc.pair_score(hd, hs, ptr=blk.ptr, idx=blk.idx, src=blk.src_nodes, **kw)
        assert want.shape[0] == blk.num_edges and same_bits(blk.score(hd, hs, **kw), want)
        gd, gs = hd[blk.src_nodes.long()].contiguous(), hs[blk.src_nodes.long()].contiguous()     # the gathered operands, direct ids
        assert same_bits(blk.score(gd, gs, gathered=True, **kw), want)
        assert same_bits(blk.score(hd, **kw), gnc.pair_score(hd, hd, ptr=blk.ptr, idx=blk.idx, src=blk.src_nodes, **kw))
